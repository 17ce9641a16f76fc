"""The umT5 text encoder on the HIP kernels (csrc/t5.hip, lightx2v_amd/t5.py) against
  * fp64 torch math for the weight-streaming bf16 GEMM (every epilogue) and the head-dim-64 attention with the relative-position bias,
  * the fixture generated from the unmodified reference (tests/golden/t5_encoder_tiny.*.safetensors) with the plain-PyTorch restatement
    (tests/t5_restatement.py, pinned to that fixture bit for bit) in fp64 as the truth, and, at the released widths, the restatement run in fp32 and in bf16
    (each prompt padded to 512, as the reference runs it) on the same GPU.
Whole-encoder bar: the project's fp32 triangle, err(HIP vs truth) <= 1.5 x err(reference bf16 vs truth) in relative L2 per prompt, plus rel L2(HIP vs reference
bf16) <= 2 x err(reference bf16 vs truth).  Measured numbers are appended to the parity summary (tests/util.py::record)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ULP_BF16 = 2.0**-7  # the widest relative spacing of bf16 (an ulp at the bottom of a binade)
FLIP_SHARE = 2e-3  # the project's share of rounding-boundary flips (tests/test_gpu_clip.py::FLIP_SHARE)
BF = torch.bfloat16


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x**3)))


def _ulp_check(got, ref64, what):
    """|got - bf16(ref64)| <= 2^-7 |ref| + 2^-24 except for FLIP_SHARE of the elements; returns the share outside."""
    ref = ref64.to(BF).double()
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bad = ((got - ref).abs() > ULP_BF16 * ref.abs() + 2.0**-24).double().mean().item()
    print(f"{what}: share outside 1 ulp {bad:.2e}, max |d| {(got - ref).abs().max().item():.3e}")
    assert bad <= FLIP_SHARE, f"{what}: {bad:.2e} of elements outside 1 ulp + 2^-24; max |d| {(got - ref).abs().max().item():.3e}"
    return bad


# (output columns N, K, GEGLU): the encoder's four Linears at the released and at the tiny widths, and an N tail that is not a multiple of 16
GEMM_SHAPES = [(12288, 4096, False), (4096, 4096, False), (4096, 10240, False), (10240, 4096, True), (768, 256, False), (640, 256, True), (256, 640, False), (484, 96, False)]


@pytest.mark.parametrize("N, K, geglu", GEMM_SHAPES)
def test_gemm_rows_bf16_every_epilogue(N, K, geglu):
    """x2v_gemm_rows_bf16 vs fp64 math with the entry's rounding points, for M = 1, 37, 203, 300, 1024, into a NaN-poisoned oversized buffer:
    NONE bf16(acc64); RESIDUAL bf16(resid + bf16(acc64)); GEGLU bf16(bf16(acc64_fc1) * gelu_tanh(bf16(acc64_gate))) from a [2N, K] weight with the rows
    interleaved.  Bar: 1 bf16 ulp (2^-7 relative) + 2^-24 outside of at most 2e-3 of the elements.  An fp32 accumulation that lands on the other side of an
    inner rounding than fp64 moves y by an ulp of the Linear output, which can be several ulps of a cancelling sum or product: with x ~ N(0, 1),
    W ~ N(0, 1 / K), resid ~ N(0, 4) an fp32 matmul on the CPU leaves 2.6e-5 (NONE), 1.1e-4 (RESIDUAL) and 4.2e-5 (GEGLU) of the elements outside at worst
    over these shapes (measured before the kernel was run; M <= 300 at the three 4096-wide shapes, every M at the others), inside the 2e-3 share."""
    from lightx2v_amd import lib
    from tests.util import record

    g = torch.Generator().manual_seed(N * 7 + K + geglu)
    rows = 2 * N if geglu else N
    w = (torch.randn(rows, K, generator=g) / K**0.5).to(BF).cuda()
    worst = 0.0
    for M in (1, 37, 203, 300, 1024):
        x = torch.randn(M, K, generator=g).to(BF).cuda()
        acc = x.double() @ w.double().t()
        if geglu:
            cases = [(lib.EPIR_GEGLU, None, acc[:, 0::2].to(BF).double() * _gelu64(acc[:, 1::2].to(BF).double()), "geglu")]
        else:
            resid = (torch.randn(M, N, generator=g) * 2).to(BF).cuda()
            cases = [(lib.EPIR_NONE, None, acc, "none"), (lib.EPIR_RESIDUAL, resid, resid.double() + acc.to(BF).double(), "residual")]
        for epi, r, y64, what in cases:
            store = torch.full((M * N + 4096,), float("nan"), dtype=BF, device="cuda")
            out = store[: M * N].view(M, N)
            lib.gemm_rows_bf16(x, w, epilogue=epi, resid=r, out=out)
            torch.cuda.synchronize()
            assert torch.isnan(store[M * N :]).all(), "gemm_rows_bf16 wrote past its output"
            worst = max(worst, _ulp_check(out, y64, f"gemm_rows_bf16 M={M} N={N} K={K} {what}"))
    record(f"gemm_rows_bf16 N={N} K={K} geglu={geglu}", worst_share_outside_1ulp=worst)


def test_gemm_rows_bf16_residual_in_place_and_packed_rows_bit_equal():
    """y may alias resid (the encoder's x = x + o(...)); the rows of an M = 203 call equal the M = 77 and M = 126 calls on the same rows, bit for bit, for
    every epilogue, across different tile choices."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(5)
    x = torch.randn(203, 4096, generator=g).to(BF).cuda()
    w = (torch.randn(4096, 4096, generator=g) / 64).to(BF).cuda()
    r = torch.randn(203, 4096, generator=g).to(BF).cuda()
    assert lib.gemm_rows_bf16_tile_choice(203, 4096) != lib.gemm_rows_bf16_tile_choice(77, 4096)
    assert lib.gemm_rows_bf16_tile_choice(203, 2048, lib.EPIR_GEGLU) != lib.gemm_rows_bf16_tile_choice(77, 2048, lib.EPIR_GEGLU)
    assert len({lib.gemm_rows_bf16_tile_choice(M, 4096) for M in (203, 126, 77)}) >= 2
    full = {epi: lib.gemm_rows_bf16(x, w, epilogue=epi, resid=r if epi == lib.EPIR_RESIDUAL else None) for epi in (lib.EPIR_NONE, lib.EPIR_RESIDUAL, lib.EPIR_GEGLU)}
    for lo, hi in ((0, 77), (77, 203)):
        part = r[lo:hi].clone()
        lib.gemm_rows_bf16(x[lo:hi], w, epilogue=lib.EPIR_RESIDUAL, resid=part, out=part)  # in place
        assert torch.equal(part, full[lib.EPIR_RESIDUAL][lo:hi])
        for epi in (lib.EPIR_NONE, lib.EPIR_GEGLU):
            assert torch.equal(lib.gemm_rows_bf16(x[lo:hi], w, epilogue=epi), full[epi][lo:hi])


def test_gemm_rows_bf16_wrapper_refusals():
    from lightx2v_amd import lib

    x = torch.zeros(8, 64, dtype=BF, device="cuda")
    w = torch.zeros(64, 64, dtype=BF, device="cuda")
    with pytest.raises(lib.X2VError, match="out / resid must be"):
        lib.gemm_rows_bf16(x, w, out=torch.empty(8, 32, dtype=BF, device="cuda"))
    with pytest.raises(lib.X2VError, match="out / resid must be"):
        lib.gemm_rows_bf16(x, w, epilogue=lib.EPIR_GEGLU, out=torch.empty(8, 64, dtype=BF, device="cuda"))  # GEGLU halves the columns
    with pytest.raises(lib.X2VError, match="resid goes with"):
        lib.gemm_rows_bf16(x, w, epilogue=lib.EPIR_RESIDUAL)
    with pytest.raises(lib.X2VError, match="disagree on K"):
        lib.gemm_rows_bf16(x, torch.zeros(64, 32, dtype=BF, device="cuda"))


# ---- attention --------------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(qkv, bias, cu, H, scale=1.0):
    """fp64 softmax(scale q . k + bias[h][j - i + 511]) v per sequence → ([rows, H * 64], max |v|)."""
    D = H * 64
    out = torch.zeros(qkv.shape[0], D, dtype=torch.float64, device=qkv.device)
    b64 = bias.double()
    for lo, hi in zip(cu, cu[1:]):
        n = hi - lo
        q, k, v = qkv[lo:hi, : 3 * D].double().view(n, 3, H, 64).unbind(1)
        idx = torch.arange(n, device=qkv.device)
        delta = idx[None, :] - idx[:, None] + 511  # [i, j]
        s = torch.einsum("ihd,jhd->hij", q, k) * scale + b64[:, delta]
        out[lo:hi] = torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1), v).reshape(n, D)
    return out


def _attn_case(H, lens, seed, q_gain=1.0):
    g = torch.Generator().manual_seed(seed)
    D, rows = H * 64, sum(lens)
    buf = torch.randn(rows, 3 * D + 16, generator=g)
    buf[:, :D] *= q_gain
    buf = buf.to(BF).cuda()
    bias = torch.randn(H, 1023, generator=g).cuda()  # N(0, 1), different per head and not symmetric in the delta
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return buf[:, : 3 * D], bias, cu  # a view with row stride 3 * H * 64 + 16


def _attn_check(qkv, bias, cu, H, what):
    """Bar from the formats: the probabilities enter the PV product rounded to bf16 (so at most 2^-8 max|v| on a convex combination, with the 1.05 of the d80
    test for the fp32 statistics and the 1 / sum), and the output is rounded once (2^-7 |ref|, the widest bf16 spacing): |d| <= 2^-7 |ref| + 1.05 * 2^-8
    max|v| on every element, no share.  The kernel rounds nowhere else."""
    from lightx2v_amd import lib
    from tests.util import record

    rows, D = qkv.shape[0], H * 64
    store = torch.full((rows * D + 4096,), float("nan"), dtype=BF, device="cuda")
    out = store[: rows * D].view(rows, D)
    lib.attention_bf16_d64_relbias(qkv, bias, cu, H, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(store[rows * D :]).all(), "the attention kernel wrote past its output"
    assert torch.isfinite(out).all(), f"{what}: non-finite output (a row of a sequence not written, or an overflow)"
    ref = _attn_ref(qkv, bias, cu, H)
    d = (out.double() - ref).abs()
    tol = ULP_BF16 * ref.abs() + 1.05 * 2.0**-8 * qkv[:, 2 * D :].double().abs().max()
    print(f"{what}: max |d| {d.max().item():.3e}, worst excess {(d - tol).max().item():.3e}, rel L2 {_rel(out, ref):.3e}")
    record(what, max_abs=d.max().item(), rel_l2=_rel(out, ref))
    assert (d <= tol).all(), f"{what}: max |d| {d.max().item():.3e}, worst excess {(d - tol).max().item():.3e}"
    return out


@pytest.mark.parametrize("H", [4, 64])
@pytest.mark.parametrize("lens", [(1,), (17,), (64,), (65,), (130,), (512,), (37, 64, 1, 130)])
def test_attention_bf16_d64_relbias(H, lens):
    """x2v_attn_bf16_d64_relbias vs fp64 attention with the bias added to the scores, on a strided QKV buffer, at the edges of the key-tile classes
    (64 | 65, 128 | 130, 512), a single token, and a packed batch of four unequal sequences."""
    qkv, bias, cu = _attn_case(H, lens, 100 * H + sum(lens))
    _attn_check(qkv, bias, cu, H, f"attn_bf16_d64_relbias H={H} lens={lens}")


def test_attention_large_scores_stay_finite():
    """q scaled by 4: |scores| reach ~100 without a softmax scale, exp of which overflows fp32 unless the row maximum is subtracted."""
    qkv, bias, cu = _attn_case(4, (130, 77), 9, q_gain=4.0)
    D = 256
    s = torch.einsum("ihd,jhd->hij", qkv[:130, :D].double().view(130, 4, 64), qkv[:130, D : 2 * D].double().view(130, 4, 64))
    assert s.abs().max() > 89, "the case must exceed log(fp32 max)"
    _attn_check(qkv, bias, cu, 4, "attn_bf16_d64_relbias q x 4")


def test_attention_never_reads_rows_outside_the_sequence():
    """Two sequences with junk rows behind each (cu_seqlens may start anywhere): filling the junk with 1e4 or with zeros gives the same bits, and the junk
    rows of the output are not written."""
    from lightx2v_amd import lib

    H, D = 4, 256
    g = torch.Generator().manual_seed(3)
    base = torch.randn(320, 3 * D, generator=g).to(BF).cuda()
    bias = torch.randn(H, 1023, generator=g).cuda()
    spans, outs = ((0, 77), (128, 254)), []
    for fill in (1e4, 0.0):
        qkv = base.clone()
        qkv[77:128], qkv[254:] = fill, fill
        out = torch.full((320, D), float("nan"), dtype=BF, device="cuda")
        for lo, hi in spans:
            lib.attention_bf16_d64_relbias(qkv, bias, [lo, hi], H, out=out)
        assert torch.isnan(out[77:128]).all() and torch.isnan(out[254:]).all() and torch.isfinite(out[:77]).all() and torch.isfinite(out[128:254]).all()
        outs.append(out)
    assert torch.equal(outs[0][:77], outs[1][:77]) and torch.equal(outs[0][128:254], outs[1][128:254])


def test_attention_packed_equals_single_sequences():
    from lightx2v_amd import lib

    for H in (4, 64):
        qkv, bias, cu = _attn_case(H, (77, 126), 11 + H)
        packed = lib.attention_bf16_d64_relbias(qkv, bias, cu, H)
        a = lib.attention_bf16_d64_relbias(qkv[:77], bias, [0, 77], H)
        b = lib.attention_bf16_d64_relbias(qkv[77:], bias, [0, 126], H)
        assert torch.equal(packed[:77], a) and torch.equal(packed[77:], b)


def test_attention_wrapper_refusals():
    from lightx2v_amd import lib

    qkv = torch.zeros(600, 768, dtype=BF, device="cuda")
    bias = torch.zeros(4, 1023, device="cuda")
    with pytest.raises(lib.X2VError, match="out must be"):
        lib.attention_bf16_d64_relbias(qkv, bias, [0, 8], 4, out=torch.empty(600, 128, dtype=BF, device="cuda"))
    with pytest.raises(lib.X2VError, match="is not"):
        lib.attention_bf16_d64_relbias(qkv[:, :512], bias, [0, 8], 4)  # a column slice: q | k without v
    with pytest.raises(lib.X2VError, match="batch <= 8"):
        lib.attention_bf16_d64_relbias(qkv, bias, list(range(0, 40, 4)), 4)
    with pytest.raises(lib.X2VError, match="length <= 512"):
        lib.attention_bf16_d64_relbias(qkv, bias, [0, 513], 4)
    with pytest.raises(lib.X2VError, match="increase"):
        lib.attention_bf16_d64_relbias(qkv, bias, [0, 8, 8], 4)
    with pytest.raises(lib.X2VError, match="rows"):
        lib.attention_bf16_d64_relbias(qkv, bias, [0, 400, 601], 4)
    with pytest.raises(lib.X2VError, match="expected 4092 elements"):
        lib.attention_bf16_d64_relbias(qkv, torch.zeros(4, 1022, device="cuda"), [0, 8], 4)


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("t5_encoder_tiny")


@pytest.fixture(scope="module")
def tiny(gold):
    from lightx2v_amd import synth, t5

    sd = synth.synth_t5_weights(synth.T5_DIMS["t5-tiny"], seed=int(gold["seed"][0]))
    return sd, t5.T5EncoderModel(512, torch.bfloat16, "cuda", sd)


def _triangle(hip, ref16, truth, what):
    from tests.util import record

    e_hip, e_ref, e_pair = _rel(hip, truth), _rel(ref16, truth), _rel(hip, ref16)
    print(f"{what}: HIP vs truth {e_hip:.3e}; reference bf16 vs truth {e_ref:.3e}; HIP vs reference bf16 {e_pair:.3e}")
    record(what, hip_vs_truth=e_hip, ref_bf16_vs_truth=e_ref, hip_vs_ref_bf16=e_pair)
    assert torch.isfinite(hip.float()).all()
    assert e_hip <= 1.5 * e_ref, f"{what}: err(HIP) {e_hip:.3e} > 1.5 x err(reference bf16) {e_ref:.3e}"
    assert e_pair <= 2 * e_ref, f"{what}: HIP vs reference bf16 {e_pair:.3e} > 2 x err(reference bf16) {e_ref:.3e}"


def test_encoder_vs_reference_fixture(gold, tiny):
    """t5-tiny (256 / 4 heads / 640 / 2 blocks) on the fixture's four prompts (37, 64, 1 and 130 valid tokens of 136) in one packed pass, against the
    reference's bf16 outputs with the fp64 restatement as the truth."""
    from tests import t5_restatement as R

    sd, m = tiny
    outs = m.infer_ids(gold["ids"], gold["mask"])
    truth = R.infer_ids(sd, gold["ids"], gold["mask"], dtype=torch.float64)
    assert len(outs) == 4
    for b, (o, n) in enumerate(zip(outs, (37, 64, 1, 130))):
        assert tuple(o.shape) == (n, 256) and o.dtype == torch.bfloat16 and o.is_cuda
        _triangle(o, gold[f"out_{b}"], truth[b], f"t5 tiny encoder prompt {b} ({n} tokens)")
    again = m.infer_ids(gold["ids"][1:2], gold["mask"][1:2])  # alone: the same bits as inside the packed pass
    assert torch.equal(again[0], outs[1])
    from lightx2v_amd import t5

    fresh = t5.T5EncoderModel(512, torch.bfloat16, "cuda", sd)  # smallest pass first: the workspace grows between the calls
    assert torch.equal(fresh.infer_ids(gold["ids"][2:3], gold["mask"][2:3])[0], outs[2])
    assert all(torch.equal(a, b) for a, b in zip(fresh.infer_ids(gold["ids"], gold["mask"]), outs)) and fresh._rows == 232


def test_encoder_released_widths():
    """4096 / 64 heads / 10 240 with 2 blocks and a vocabulary of 1024, weights drawn on the GPU, prompts of 77 and 126 tokens, against the restatement run
    on the same GPU in fp32 (truth) and in bf16 with each prompt padded to 512 (what the reference computes); run_text_encoder's one packed pass equals two
    separate infer_ids calls bit for bit."""
    from lightx2v_amd import synth, t5
    from tests import t5_restatement as R

    dims = dict(synth.T5_DIMS["umt5-xxl"], vocab=1024, layers=2)
    sd = synth.synth_t5_weights(dims, seed=2, device="cuda")
    m = t5.T5EncoderModel(512, torch.bfloat16, "cuda", sd)
    assert (m.dim, m.dim_attn, m.dim_ffn, m.num_heads, m.num_layers) == (4096, 4096, 10240, 64, 2)
    g = torch.Generator().manual_seed(4)
    prompts = []
    for n in (77, 126):
        ids, mask = torch.zeros(1, n, dtype=torch.long), torch.ones(1, n, dtype=torch.long)
        ids[0] = torch.randint(1, 1024, (n,), generator=g)
        prompts.append((ids, mask))
    both = t5.run_text_encoder(m, *prompts[0], *prompts[1])
    assert len(both["context"]) == 1 and len(both["context_null"]) == 1
    for (ids, mask), packed, n in zip(prompts, (both["context"][0], both["context_null"][0]), (77, 126)):
        assert tuple(packed.shape) == (n, 4096)
        assert torch.equal(m.infer_ids(ids, mask)[0], packed), f"the {n}-token prompt alone differs from its rows in the packed pass"
        pi, pm = R.pad_to(ids, mask, 512)
        with torch.no_grad():
            truth = R.infer_ids(sd, pi, pm, dtype=torch.float32, device="cuda")[0]
            ref16 = R.infer_ids(sd, pi, pm, dtype=torch.bfloat16, device="cuda")[0]
        _triangle(packed, ref16, truth, f"t5 released widths, 2 blocks, {n} tokens")


def test_wan_forward_with_hip_context(tiny):
    """One wan-tiny conditional forward whose `context` comes from the HIP encoder.  wan-tiny's text dim is 64 (and its text_len 32), so a 24-token prompt's
    256-wide output is projected to 64 by a fixed seeded matrix (test glue); the HIP forward must be finite and agree with the oracle fed the same tokens
    at the existing forward tolerance (2e-2)."""
    from lightx2v_amd import scheduler, synth, wan
    from oracle import wan_oracle as O

    _, m = tiny
    ids = torch.randint(1, 384, (1, 24), generator=torch.Generator().manual_seed(6))
    tokens = m.infer_ids(ids, torch.ones_like(ids))[0]
    assert tokens.shape == (24, 256) and tokens.dtype == torch.bfloat16 and tokens.is_cuda
    dims = synth.WAN_DIMS["wan-tiny"]
    ts, frames = (16, 3, 8, 8), 9
    proj = torch.randn(256, dims["text_dim"], generator=torch.Generator().manual_seed(2)) / 16
    ctx = [(tokens.float().cpu() @ proj).to(torch.bfloat16)]
    wd = synth.synth_wan_weights(dims, seed=0)
    lat, _, _ = synth.synth_inputs(dims, ts)
    cfg = wan.default_config(dims, target_shape=ts, target_video_length=frames, infer_steps=2)
    model = wan.WanModel(cfg, {k: v.cuda() for k, v in wd.items()})
    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": []}}
    sch.step_pre(0)
    got = model._forward(inputs, True)
    assert torch.isfinite(got.float()).all()
    with torch.no_grad():
        ref = O.wan_forward(wd, dims, lat.to(torch.bfloat16), sch.timesteps[0].cpu(), ctx)
    e = _rel(got, ref)
    assert e <= 2e-2, f"wan-tiny forward with HIP T5 context vs oracle: relative L2 {e:.3e}"
