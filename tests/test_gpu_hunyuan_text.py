"""HunyuanVideo's two text towers on the HIP kernels (csrc/txt_enc.hip, lightx2v_amd/llama.py, lightx2v_amd/clip_text.py) against
  * fp64 torch math with each entry's rounding points for the causal attention, the two new fp16 GEMM epilogues and the fp16 RMSNorm,
  * the fixtures stored from transformers' models (tests/golden/llama_encoder_tiny, clip_text_tiny) with the plain-PyTorch restatements
    (tests/llama_restatement.py, tests/clip_text_restatement.py) in fp64 as the truth, and, at the released widths, the restatements run in fp32 and in
    fp16 on the same GPU, padded as the reference runs them.
Whole-tower bar: the project's fp32 triangle, err(HIP vs truth) <= 1.5 x err(reference fp16 vs truth) in relative L2 per prompt, plus rel L2(HIP vs
reference fp16) <= 2 x err(reference fp16 vs truth).  Measured numbers are appended to the parity summary (tests/util.py::record)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP16 = 2.0**-10  # the widest relative spacing of fp16 (an ulp at the bottom of a binade)
FLIP_SHARE = 2e-3  # the project's share of rounding-boundary flips (tests/test_gpu_clip.py::FLIP_SHARE)
F16 = torch.float16


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---- x2v_attn_f16_causal -----------------------------------------------------------------------------------------------------------------------------------
MODES = [(128, True), (128, False), (64, False)]  # (head_dim, rope)
HEADS = [(4, 1), (4, 2), (8, 8)]
SEQS = [(1,), (63,), (64,), (65,), (127,), (128,), (129,), (351,), (512,), (1, 64, 65), (351, 130), (33,) * 8]


@pytest.fixture(scope="module")
def rope():
    from lightx2v_amd.llama import rope_tables

    return tuple(t.cuda() for t in rope_tables(500000.0))


def _attn_reference(qkv, cu, H, Hkv, d, rope):
    """fp64 causal grouped-query attention per sequence with the kernel's rounding points: q and k rotated in fp64 from the fp16 inputs and the fp32 tables,
    rounded to fp16; everything after that in fp64.  Returns (ref [rows, H * d] with NaN outside the sequences, max |v|)."""
    rows = qkv.shape[0]
    ref = torch.full((rows, H * d), float("nan"), dtype=torch.float64, device=qkv.device)
    group = H // Hkv
    for a, b in zip(cu, cu[1:]):
        n = b - a
        x = qkv[a:b].double()
        q, k, v = x[:, : H * d].view(n, H, d), x[:, H * d : (H + Hkv) * d].view(n, Hkv, d), x[:, (H + Hkv) * d : (H + 2 * Hkv) * d].view(n, Hkv, d)
        if rope is not None:
            cos, sin = (torch.cat([t[:n].double(), t[:n].double()], dim=-1)[:, None] for t in rope)

            def rot(t):
                return (t * cos + torch.cat([-t[..., d // 2 :], t[..., : d // 2]], dim=-1) * sin).to(F16).double()

            q, k = rot(q), rot(k)
        kv_of = [h // group for h in range(H)]
        s = torch.einsum("ihd,jhd->hij", q, k[:, kv_of]) * d**-0.5
        s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=qkv.device).tril(), float("-inf"))
        ref[a:b] = torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1), v[:, kv_of]).reshape(n, H * d)
    return ref


def _run_attention(lens, H, Hkv, d, rope, seed):
    """One launch on a strided qkv whose rows outside the sequences hold 1e4, into a NaN-poisoned oversized buffer; returns (out, ref, max |v|)."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(seed)
    cols = (H + 2 * Hkv) * d
    cu = [3]
    for n in lens:
        cu.append(cu[-1] + n)
    rows = cu[-1] + 5
    buf = torch.full((rows, cols + 16), 1e4, dtype=F16)
    buf[cu[0] : cu[-1]] = torch.randn(cu[-1] - cu[0], cols + 16, generator=g).half()
    buf = buf.cuda()
    qkv = buf[:, :cols]
    store = torch.full((rows * H * d + 4096,), float("nan"), dtype=F16, device="cuda")
    out = store[: rows * H * d].view(rows, H * d)
    lib.attention_f16_causal(qkv, cu, H, Hkv, d, rope=rope, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(store[rows * H * d :]).all(), "the attention kernel wrote past its output"
    assert torch.isnan(out[: cu[0]]).all() and torch.isnan(out[cu[-1] :]).all(), "the attention kernel wrote rows outside every sequence"
    ref = _attn_reference(qkv, cu, H, Hkv, d, rope)
    vmax = qkv[cu[0] : cu[-1], (H + Hkv) * d :].double().abs().max().item()
    return out[cu[0] : cu[-1]].double(), ref[cu[0] : cu[-1]], vmax


def _attn_check(out, ref, vmax, what):
    """|d| <= 2^-10 |ref| + 2^-11 max|v| on every element: the probabilities enter the PV product rounded to fp16 (relative 2^-11 each, so at most
    2^-11 max|v| on a convex combination) and the output is rounded once (2^-11 |o|); fp32 softmax statistics add ~1e-6."""
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    d = (out - ref).abs()
    tol = ULP16 * ref.abs() + 2.0**-11 * vmax
    worst = (d / tol).max().item()
    print(f"{what}: max |d| {d.max().item():.3e}, worst |d| / bar {worst:.3f}")
    assert (d <= tol).all(), f"{what}: max |d| {d.max().item():.3e}, worst excess {(d - tol).max().item():.3e} (|d| / bar {worst:.3f})"
    return worst


@pytest.mark.parametrize("lens", SEQS, ids=lambda s: "+".join(str(n) for n in s))
def test_attention_f16_causal_vs_fp64(lens, rope):
    """Every sequence shape at which a branch of the kernel can go wrong — one token, one short of / exactly / one past one and two key tiles, the
    released 351, the 512 limit, packed batches with a one-token and a tile-sized sequence, and the batch limit of 8 — with (d = 128, rope), (d = 128, no
    rope) and (d = 64), for 4 / 1, 4 / 2 and 8 / 8 query / key-value heads."""
    from tests.util import record

    worst = 0.0
    for d, with_rope in MODES:
        for H, Hkv in HEADS:
            out, ref, vmax = _run_attention(lens, H, Hkv, d, rope if with_rope else None, seed=sum(lens) * 13 + d + H + Hkv)
            worst = max(worst, _attn_check(out, ref, vmax, f"attn_f16_causal lens={lens} d={d} rope={with_rope} H={H}/{Hkv}"))
    record(f"attn_f16_causal lens={lens}", worst_share_of_bar=worst)


def test_attention_f16_causal_released_heads(rope):
    """32 query heads over 8 key/value heads at 351 tokens: the Llama tower's launch."""
    from tests.util import record

    out, ref, vmax = _run_attention((351,), 32, 8, 128, rope, seed=7)
    record("attn_f16_causal 351 tokens 32/8 heads", worst_share_of_bar=_attn_check(out, ref, vmax, "attn_f16_causal 351 tokens H=32/8 rope"))


@pytest.mark.parametrize("d, n", [(128, 130), (64, 70)])
def test_attention_f16_causal_sharp_diagonal(d, n):
    """q = 0 (every allowed key weighs 1 / (i + 1)) and V = one-hot rows (key j lights column j mod d): output row i is the histogram of the keys <= i over
    i + 1.  A diagonal tile masked one key late leaks into column i + 1, which must be exactly 0 for i + 1 < d; one key early loses column i."""
    from lightx2v_amd import lib

    H = 2
    qkv = torch.zeros(n, 3 * H * d, dtype=F16)
    qkv[:, H * d : 2 * H * d] = torch.randn(n, H * d, generator=torch.Generator().manual_seed(1)).half()
    for j in range(n):
        for h in range(H):
            qkv[j, 2 * H * d + h * d + j % d] = 1.0
    out = lib.attention_f16_causal(qkv.cuda(), [0, n], H, H, d).double().cpu().view(n, H, d)
    want = torch.zeros(n, d, dtype=torch.float64)
    for i in range(n):
        want[i] = torch.bincount(torch.arange(i + 1) % d, minlength=d).double() / (i + 1)
    for h in range(H):
        assert ((out[:, h] == 0) == (want == 0)).all(), "a key behind the query contributed, or a key up to the query did not"
        assert ((out[:, h] - want).abs() <= ULP16 * want + 1e-6).all()
    from tests.util import record

    record(f"attn_f16_causal sharp diagonal d={d}", max_abs=(out - want[:, None]).abs().max().item())


def test_attention_f16_causal_wrapper_refusals(rope):
    from lightx2v_amd import lib

    qkv = torch.zeros(16, 3 * 128, dtype=F16, device="cuda")
    with pytest.raises(lib.X2VError, match="is not"):
        lib.attention_f16_causal(qkv, [0, 16], 2, 1, 128)
    with pytest.raises(lib.X2VError, match="ends at row"):
        lib.attention_f16_causal(qkv, [0, 17], 1, 1, 128)
    with pytest.raises(lib.X2VError, match="head_dim 128 only"):
        lib.attention_f16_causal(qkv[:, :192], [0, 16], 1, 1, 64, rope=rope)
    with pytest.raises(lib.X2VError, match="rope tables"):
        lib.attention_f16_causal(qkv, [0, 16], 1, 1, 128, rope=(rope[0][:100], rope[1][:100]))


# ---- x2v_gemm_f16: the new epilogues -----------------------------------------------------------------------------------------------------------------------
def _ulp_check(got, ref64, what, atol):
    """|got - fp16(ref64)| <= 2^-10 |ref| + atol except for FLIP_SHARE of the elements; returns the share outside."""
    ref = ref64.to(F16).double()
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bad = ((got - ref).abs() > ULP16 * ref.abs() + atol).double().mean().item()
    print(f"{what}: share outside 1 ulp {bad:.2e}, max |d| {(got - ref).abs().max().item():.3e}")
    assert bad <= FLIP_SHARE, f"{what}: {bad:.2e} of elements outside 1 ulp + {atol}; max |d| {(got - ref).abs().max().item():.3e}"
    return bad


# (output columns N, K, SwiGLU): the Llama gate | up Linear at the released and the tiny widths, CLIP-L's fc1, and an N tail that is not a multiple of 16 for each
EPI_SHAPES = [(14336, 4096, True), (448, 512, True), (3072, 768, False), (452, 512, True), (3076, 768, False)]


@pytest.mark.parametrize("N, K, swiglu", EPI_SHAPES)
def test_gemm_f16_quick_gelu_and_swiglu(N, K, swiglu):
    """x2v_gemm_f16 with the two new epilogues vs fp64 math with the entry's rounding points, for M = 1, 37, 351, 1024 (rows of one M = 1024 operand, whose
    fp64 product is computed once), into a NaN-poisoned oversized buffer: QUICK_GELU fp16(v * sigmoid(1.702 v)), v = acc64 + bias; SWIGLU
    fp16(silu(fp16(acc64_gate)) * fp16(acc64_up)) from a [2N, K] weight with the rows interleaved.  Bar: 1 fp16 ulp + 2^-23 outside of at most 2e-3 of
    the elements (an fp32 accumulation that lands on the other side of an inner rounding than fp64 moves a factor by one ulp)."""
    from lightx2v_amd import lib
    from tests.util import record

    g = torch.Generator().manual_seed(N * 7 + K + swiglu)
    w = (torch.randn(2 * N if swiglu else N, K, generator=g) / K**0.5).half().cuda()
    bias = None if swiglu else (torch.randn(N, generator=g) * 0.1).half().cuda()
    x = torch.randn(1024, K, generator=g).half().cuda()
    acc = x.double() @ w.double().t()
    if swiglu:
        gate, up = acc[:, 0::2].to(F16).double(), acc[:, 1::2].to(F16).double()
        y64 = gate * torch.sigmoid(gate) * up
    else:
        v = acc + bias.double()
        y64 = v * torch.sigmoid(1.702 * v)
    del acc
    worst = 0.0
    for M in (1, 37, 351, 1024):
        store = torch.full((M * N + 4096,), float("nan"), dtype=F16, device="cuda")
        out = store[: M * N].view(M, N)
        lib.gemm_f16(x[:M], w, bias, epilogue=lib.EPI16_SWIGLU if swiglu else lib.EPI16_QUICK_GELU, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(store[M * N :]).all(), "gemm_f16 wrote past its output"
        worst = max(worst, _ulp_check(out, y64[:M], f"gemm_f16 M={M} N={N} K={K} {'swiglu' if swiglu else 'quick_gelu'}", 2.0**-23))
    record(f"gemm_f16 new epilogue N={N} K={K} swiglu={swiglu}", worst_share_outside_1ulp=worst)


def test_gemm_f16_earlier_epilogues_keep_their_bits():
    """Epilogues 0..2 on one shape (M = 300, N = 3072, K = 768, with bias) after the kernel gained two more.  Only this tree's library is at hand here, so
    what they wrote before is recomputed from the entry itself as far as that can be done; every output value is one lane's k-ordered reduction whatever
    the tile, so
      * NONE on the rows alone (M = 37: another tile) equals the same rows of the M = 300 call, bit for bit;
      * RESIDUAL equals fp16(resid + NONE's output) formed by torch in fp32 (the sum of two fp16 values is exact there, so the one rounding is the
        kernel's), bit for bit;
      * GELU_ERF is held to fp16(gelu_erf(v)) within the 1 ulp + 2^-23 of tests/test_gpu_clip.py — not to bits, which nothing here can supply — and its
        M = 37 rows equal the M = 300 call's bit for bit;
      * the three are run again after a SwiGLU and a quick-GELU launch on the same operands and give the same bits: run-to-run determinism only.
    The comparison against the previous build of the library itself (same inputs, equal bits for these three and for the bf16 instantiation's three) was
    recorded once, in profiles/hunyuan_text_gemm_f16_bits_vs_parent.txt."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(11)
    M, N, K = 300, 3072, 768
    x = torch.randn(M, K, generator=g).half().cuda()
    w = (torch.randn(N, K, generator=g) / K**0.5).half().cuda()
    bias = (torch.randn(N, generator=g) * 0.1).half().cuda()
    resid = (torch.randn(M, N, generator=g) * 2).half().cuda()

    def three():
        return (lib.gemm_f16(x, w, bias), lib.gemm_f16(x, w, bias, epilogue=lib.EPI16_GELU_ERF), lib.gemm_f16(x, w, bias, epilogue=lib.EPI16_RESIDUAL, resid=resid))

    none, gelu, res = three()
    assert torch.equal(lib.gemm_f16(x[:37], w, bias), none[:37]) and torch.equal(lib.gemm_f16(x[:37], w, bias, epilogue=lib.EPI16_GELU_ERF), gelu[:37])
    assert torch.equal(res, (resid.float() + none.float()).half())
    v = x.double() @ w.double().t() + bias.double()
    _ulp_check(gelu, torch.nn.functional.gelu(v), "gemm_f16 gelu_erf after the change", 2.0**-23)
    _ulp_check(none, v, "gemm_f16 none after the change", 2.0**-23)
    lib.gemm_f16(x, w, None, epilogue=lib.EPI16_SWIGLU)
    lib.gemm_f16(x, w, bias, epilogue=lib.EPI16_QUICK_GELU)
    assert all(torch.equal(a, b) for a, b in zip(three(), (none, gelu, res)))


# ---- x2v_rmsnorm_f16 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, D", [(1, 512), (351, 512), (1, 4096), (351, 4096)])
def test_rmsnorm_f16(M, D):
    """fp64 RMSNorm rounded once, 1 ulp + 1e-5, on a strided input into a strided NaN-poisoned output."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(M + D)
    xs = (torch.randn(M, D + 8, generator=g) * 2 + 0.5).half().cuda()
    w = (1 + 0.1 * torch.randn(D, generator=g)).half().cuda()
    store = torch.full((M, D + 16), float("nan"), dtype=F16, device="cuda")
    lib.rmsnorm_f16(xs[:, :D], w, eps=1e-5, out=store[:, :D])
    torch.cuda.synchronize()
    assert torch.isnan(store[:, D:]).all()
    x = xs[:, :D].double()
    from tests.util import record

    record(f"rmsnorm_f16 {M}x{D}", share_outside_1ulp=_ulp_check(store[:, :D], w.double() * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5), f"rmsnorm_f16 {M}x{D}", 1e-5))


# ---- whole towers --------------------------------------------------------------------------------------------------------------------------------------------
def _triangle(hip, ref16, truth, what):
    from tests.util import record

    e_hip, e_ref, e_pair = _rel(hip, truth), _rel(ref16, truth), _rel(hip, ref16)
    print(f"{what}: HIP vs truth {e_hip:.3e}; reference fp16 vs truth {e_ref:.3e}; HIP vs reference fp16 {e_pair:.3e}")
    record(what, hip_vs_truth=e_hip, ref_fp16_vs_truth=e_ref, hip_vs_ref_fp16=e_pair)
    assert torch.isfinite(hip.float()).all()
    assert e_hip <= 1.5 * e_ref, f"{what}: err(HIP) {e_hip:.3e} > 1.5 x err(reference fp16) {e_ref:.3e}"
    assert e_pair <= 2 * e_ref, f"{what}: HIP vs reference fp16 {e_pair:.3e} > 2 x err(reference fp16) {e_ref:.3e}"


@pytest.fixture(scope="module")
def llama_tiny():
    from lightx2v_amd import llama, synth
    from tests import llama_restatement as R
    from tests.util import load_golden

    gold = load_golden("llama_encoder_tiny")
    dims = synth.LLAMA_DIMS["llama-tiny"]
    sd = synth.synth_llama_weights(dims, seed=int(gold["seed"][0]))
    with torch.no_grad():
        truth = R.infer_ids(sd, dims, gold["ids"], gold["mask"], dtype=torch.float64)[0]
    return gold, (sd, dims), truth, llama.TextEncoderHFLlamaModel((sd, dims), "cuda")


@pytest.fixture(scope="module")
def clip_tiny():
    from lightx2v_amd import clip_text, synth
    from tests import clip_text_restatement as R
    from tests.util import load_golden

    gold = load_golden("clip_text_tiny")
    dims = synth.CLIP_TEXT_DIMS["clip-text-tiny"]
    sd = synth.synth_clip_text_weights(dims, seed=int(gold["seed"][0]))
    with torch.no_grad():
        truth = R.infer_ids(sd, dims, gold["ids"], gold["mask"], dtype=torch.float64)[0]
    return gold, (sd, dims), truth, clip_text.TextEncoderHFClipModel((sd, dims), "cuda")


def test_llama_tower_vs_reference_fixture(llama_tiny):
    """The tiny tower (512 wide, 4 / 2 heads of 128, 2 of 4 layers) on the four fixture prompts (96, 97, 130, 136 valid tokens of 136): the triangle on the
    valid rows against the reference's fp16 output; padded rows exactly zero, the cropped mask returned unchanged; a prompt run alone on a fresh model and
    after a longer one gives the same bits (workspace reuse)."""
    from lightx2v_amd import llama

    gold, model_args, truth, m = llama_tiny
    lens = gold["mask"].sum(1).tolist()
    outs = {}
    for b in (3, 0, 1, 2):  # the longest first: the later ones run in a larger workspace
        n = lens[b]
        states, mask = m.infer_ids(gold["ids"][b : b + 1], gold["mask"][b : b + 1])
        assert states.shape == (1, 41, 512) and states.dtype == F16 and states.is_cuda
        assert torch.equal(mask.cpu(), gold["mask"][b : b + 1, 95:])
        assert not states[0, n - 95 :].any(), "rows of padded tokens must be exactly zero"
        _triangle(states[0, : n - 95], gold["out_f16"][b, : n - 95], truth[b, : n - 95], f"llama tiny tower prompt {b} ({n} tokens)")
        outs[b] = states
    fresh = llama.TextEncoderHFLlamaModel(model_args, "cuda")
    assert torch.equal(fresh.infer_ids(gold["ids"][:1], gold["mask"][:1])[0], outs[0]) and fresh._rows == 96
    assert torch.equal(m.infer_ids(gold["ids"][:1, :100], gold["mask"][:1, :100])[0], outs[0][:, :5]), "padding length changed valid rows"


def test_clip_text_tower_vs_reference_fixture(clip_tiny):
    """The tiny tower (256 wide, 4 heads of 64, 4 layers) on the four fixture prompts (end token at 0, 1, 20, 76): the triangle on the pooled vector."""
    from lightx2v_amd import clip_text

    gold, model_args, truth, m = clip_tiny
    outs = {}
    for b in (3, 0, 1, 2):
        pooled, mask = m.infer_ids(gold["ids"][b : b + 1], gold["mask"][b : b + 1])
        assert pooled.shape == (1, 256) and pooled.dtype == F16 and pooled.is_cuda and torch.equal(mask, gold["mask"][b : b + 1])
        _triangle(pooled[0], gold["out_f16"][b], truth[b], f"clip text tiny tower prompt {b}")
        outs[b] = pooled
    fresh = clip_text.TextEncoderHFClipModel(model_args, "cuda")
    assert torch.equal(fresh.infer_ids(gold["ids"][2:3], gold["mask"][2:3])[0], outs[2]) and fresh._rows == 21


def test_llama_tower_released_widths():
    """4096 / 32 over 8 heads / 14 336 with 4 layers in the dict (2 run) and a vocabulary of 1024, weights drawn on the GPU, prompts of 351 and 130 valid
    tokens padded to 351, against the restatement run on the same GPU in fp32 (truth) and in fp16 (what the reference computes)."""
    from lightx2v_amd import llama, synth
    from tests import llama_restatement as R

    dims = dict(synth.LLAMA_DIMS["llama3-8b"], vocab=1024, layers=4)
    sd = synth.synth_llama_weights(dims, seed=2, device="cuda")
    m = llama.TextEncoderHFLlamaModel((sd, dims), "cuda")
    assert (m.dim, m.num_heads, m.num_kv_heads, m.dim_ffn, m.num_layers) == (4096, 32, 8, 14336, 2)
    g = torch.Generator().manual_seed(4)
    for n in (351, 130):
        ids, mask = torch.zeros(1, 351, dtype=torch.long), torch.zeros(1, 351, dtype=torch.long)
        ids[0, :n], mask[0, :n] = torch.randint(1, 1024, (n,), generator=g), 1
        states, cropped = m.infer_ids(ids, mask)
        assert states.shape == (1, 256, 4096) and torch.equal(cropped, mask[:, 95:]) and not states[0, n - 95 :].any()
        with torch.no_grad():
            truth = R.infer_ids(sd, dims, ids, mask, dtype=torch.float32, device="cuda")[0]
            ref16 = R.infer_ids(sd, dims, ids, mask, dtype=F16, device="cuda")[0]
        _triangle(states[0, : n - 95], ref16[0, : n - 95], truth[0, : n - 95], f"llama released widths, 2 layers, {n} tokens")


def test_clip_text_tower_released_widths():
    """768 / 12 heads / 3072 with 2 layers, weights drawn on the GPU, end token at 76 and at 20 (77 and 21 tokens run) of 77 positions, against the
    restatement on the same GPU in fp32 (truth) and fp16."""
    from lightx2v_amd import clip_text, synth
    from tests import clip_text_restatement as R

    dims = dict(synth.CLIP_TEXT_DIMS["clip-l"], layers=2)
    sd = synth.synth_clip_text_weights(dims, seed=2, device="cuda")
    m = clip_text.TextEncoderHFClipModel((sd, dims), "cuda")
    assert (m.dim, m.num_heads, m.dim_ffn, m.num_layers) == (768, 12, 3072, 2)
    g = torch.Generator().manual_seed(5)
    end = dims["vocab"] - 1
    for p in (76, 20):
        ids, mask = torch.full((1, 77), end, dtype=torch.long), torch.zeros(1, 77, dtype=torch.long)
        ids[0, :p], mask[0, : p + 1] = torch.randint(1, end, (p,), generator=g), 1
        pooled, _ = m.infer_ids(ids, mask)
        with torch.no_grad():
            truth = R.infer_ids(sd, dims, ids, mask, dtype=torch.float32, device="cuda")[0]
            ref16 = R.infer_ids(sd, dims, ids, mask, dtype=F16, device="cuda")[0]
        _triangle(pooled[0], ref16[0], truth[0], f"clip-l released widths, 2 layers, {p + 1} tokens")


def test_run_text_encoder_feeds_hunyuan_pre_infer(llama_tiny, clip_tiny):
    """run_text_encoder's dict (bf16 states, the cropped mask) goes into HunyuanPreInfer at tiny DiT dims as it is.  With the zero rows of padded tokens
    replaced by random finite values, `vec` and the valid rows of `txt_out` keep their bits.  The padded rows of txt_out do not and cannot: the token refiner
    embeds every row of text_states (pre_infer.py:87-89), so those rows are a function of what the padded rows hold, here as in the reference.  They never
    reach the image: cu_seqlens puts them into an attention segment of their own and the output is read from the image rows.  So the consumer-side proof
    that zero padding is harmless is taken where it counts: the whole forward's noise prediction keeps its bits too."""
    from lightx2v_amd import hunyuan as hy
    from lightx2v_amd import llama, synth

    gold_l, _, _, ml = llama_tiny
    gold_c, _, _, mc = clip_tiny
    te = llama.run_text_encoder([ml, mc], gold_l["ids"][2:3], gold_l["mask"][2:3], gold_c["ids"][2:3], gold_c["mask"][2:3])
    assert set(te) == {"text_encoder_1_text_states", "text_encoder_1_attention_mask", "text_encoder_2_text_states", "text_encoder_2_attention_mask"}
    s1, m1, s2 = te["text_encoder_1_text_states"], te["text_encoder_1_attention_mask"], te["text_encoder_2_text_states"]
    n_valid = int(m1.sum())
    assert s1.shape == (1, 41, 512) and s1.dtype == torch.bfloat16 and s2.shape == (1, 256) and s2.dtype == torch.bfloat16 and n_valid == 35
    assert torch.equal(s1, ml.infer_ids(gold_l["ids"][2:3], gold_l["mask"][2:3])[0].to(torch.bfloat16))
    dims = dict(synth.HUNYUAN_DIMS["hunyuan-tiny"], text_dim=512, text_dim_2=256, text_len=41)
    wd = synth.synth_hunyuan_weights(dims, seed=0)
    cfg = hy.default_config(dims, infer_steps=4)
    model = hy.HunyuanModel(cfg, {k: v.cuda() for k, v in wd.items()})
    sch = hy.HunyuanScheduler(cfg)
    sch.prepare(synth.synth_hunyuan_inputs(dims, synth.HUNYUAN_WORKLOADS["hunyuan-tiny"]["target_shape"])[0])
    model.set_scheduler(sch)
    sch.step_pre(1)
    noisy = dict(te)
    filled = s1.clone()
    filled[0, n_valid:] = torch.randn(41 - n_valid, 512, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    noisy["text_encoder_1_text_states"] = filled
    results = []
    for inputs in ({"text_encoder_output": te}, {"text_encoder_output": noisy}):
        _, txt, vec, cu, _, _ = model.pre_infer.infer(model.pre_weight, inputs)
        model.infer(inputs)
        results.append((txt.clone(), vec.clone(), cu.tolist(), sch.noise_pred.clone()))
    (txt, vec, cu, pred), (txt2, vec2, cu2, pred2) = results
    assert torch.isfinite(txt.float()).all() and torch.isfinite(vec.float()).all() and torch.isfinite(pred.float()).all()
    assert torch.equal(vec, vec2) and cu == cu2
    assert torch.equal(txt[:n_valid], txt2[:n_valid]), "valid rows of the token refiner depend on what padded rows hold"
    assert torch.equal(pred, pred2), "the noise prediction depends on what the rows of padded text tokens hold"
