"""Host-side checks of HunyuanVideo's two text towers (no GPU):
  * the plain-torch restatements (tests/llama_restatement.py, tests/clip_text_restatement.py) compute the reference's function: in fp64 they lie within
    rel L2 1e-2 of both outputs stored from transformers' models (tests/golden/llama_encoder_tiny, clip_text_tiny; tools/gen_golden_hunyuan_text.py), and
    every single slip listed below lies beyond that cap on at least one prompt — the cap is a separation condition, not a precision claim (measured: the
    reference is 1.2e-3 (Llama) / 9e-4 (CLIP) from the fp64 restatement in fp16 and 7e-7 / 6e-7 in fp32);
  * valid rows do not depend on padding, which is what lets the HIP towers run the valid tokens only;
  * the host logic of lightx2v_amd/llama.py and clip_text.py: pooled position, rope tables, weight layout, refusals, name prefixes;
  * argument validation of the three new C entries."""
import ctypes

import pytest
import torch

CAP = 1e-2


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def llama():
    from lightx2v_amd import synth
    from tests.util import load_golden

    gold = load_golden("llama_encoder_tiny")
    dims = synth.LLAMA_DIMS["llama-tiny"]
    return gold, dims, synth.synth_llama_weights(dims, seed=int(gold["seed"][0]))


@pytest.fixture(scope="module")
def clip():
    from lightx2v_amd import synth
    from tests.util import load_golden

    gold = load_golden("clip_text_tiny")
    dims = synth.CLIP_TEXT_DIMS["clip-text-tiny"]
    return gold, dims, synth.synth_clip_text_weights(dims, seed=int(gold["seed"][0]))


def test_synth_weights_match_the_fixture_checksums(llama, clip):
    from oracle.gen_golden import weights_checksum

    for gold, _, sd in (llama, clip):
        assert torch.equal(weights_checksum(sd), gold["weights_checksum"])
    assert llama[0]["constants"].tolist() == [351, 95, 2] and clip[0]["constants"].tolist() == [77]
    assert llama[0]["mask"].sum(1).tolist() == [96, 97, 130, 136]
    assert [int(r.argmax()) for r in clip[0]["ids"]] == [0, 1, 20, 76]


def test_llama_restatement_is_the_reference_function_and_every_slip_is_not(llama):
    from tests import llama_restatement as R

    gold, dims, sd = llama
    lens = gold["mask"].sum(1).tolist()
    crop = int(gold["constants"][1])

    def errs(slip):
        out, m = R.infer_ids(sd, dims, gold["ids"], gold["mask"], dtype=torch.float64, crop_start=crop, slip=slip)
        assert torch.equal(m, gold["mask"][:, crop:])
        return [max(_rel(out[b, : n - crop], gold[k][b, : n - crop]) for k in ("out_f16", "out_f32")) for b, n in enumerate(lens)]

    e = errs(None)
    print("llama restatement fp64 vs reference, per prompt:", e)
    assert max(e) <= CAP, e
    for slip in R.SLIPS:
        e = errs(slip)
        print(f"llama slip {slip}:", e)
        assert max(e) > CAP, f"the fixture does not tell {slip} from the reference: {e}"


def test_clip_restatement_is_the_reference_function_and_every_slip_is_not(clip):
    from tests import clip_text_restatement as R

    gold, dims, sd = clip

    def errs(slip):
        out, m = R.infer_ids(sd, dims, gold["ids"], gold["mask"], dtype=torch.float64, slip=slip)
        assert torch.equal(m, gold["mask"])
        return [max(_rel(out[b], gold[k][b]) for k in ("out_f16", "out_f32")) for b in range(out.shape[0])]

    e = errs(None)
    print("clip text restatement fp64 vs reference, per prompt:", e)
    assert max(e) <= CAP, e
    for slip in R.SLIPS:
        e = errs(slip)
        print(f"clip text slip {slip}:", e)
        assert max(e) > CAP, f"the fixture does not tell {slip} from the reference: {e}"


def test_restatements_run_in_fp32_and_fp16(llama, clip):
    """The dtype parameter: fp32 and fp16 runs stay near the fp64 truth (fp16 within the cap: the reference-leg of the GPU triangle at released widths)."""
    from tests import clip_text_restatement as C
    from tests import llama_restatement as R

    gold, dims, sd = llama
    ids, mask = gold["ids"][1:2], gold["mask"][1:2]
    truth = R.infer_ids(sd, dims, ids, mask)[0][:, :2]
    for dtype, bar in ((torch.float32, 1e-5), (torch.float16, CAP)):
        out = R.infer_ids(sd, dims, ids, mask, dtype=dtype)[0][:, :2]
        assert out.dtype == dtype and _rel(out, truth) <= bar
    gold, dims, sd = clip
    truth = C.infer_ids(sd, dims, gold["ids"], gold["mask"])[0]
    for dtype, bar in ((torch.float32, 1e-5), (torch.float16, CAP)):
        out = C.infer_ids(sd, dims, gold["ids"], gold["mask"], dtype=dtype)[0]
        assert out.dtype == dtype and _rel(out, truth) <= bar


def test_valid_rows_do_not_depend_on_padding(llama, clip):
    """Llama in fp64: rows of the 136-padded run equal the unpadded run to 1e-12.  CLIP: the pooled vector of the padded run equals that of the run
    truncated at the end token."""
    from tests import clip_text_restatement as C
    from tests import llama_restatement as R

    gold, dims, sd = llama
    for b, n in enumerate(gold["mask"].sum(1).tolist()):
        padded = R.decoder(sd, dims, gold["ids"][b : b + 1], gold["mask"][b : b + 1])[:, :n]
        alone = R.decoder(sd, dims, gold["ids"][b : b + 1, :n], gold["mask"][b : b + 1, :n])
        assert (padded - alone).abs().max().item() <= 1e-12
    gold, dims, sd = clip
    for b, p in enumerate([0, 1, 20, 76]):
        padded = C.infer_ids(sd, dims, gold["ids"][b : b + 1], gold["mask"][b : b + 1])[0]
        cut = C.infer_ids(sd, dims, gold["ids"][b : b + 1, : p + 1], gold["mask"][b : b + 1, : p + 1])[0]
        assert (padded - cut).abs().max().item() <= 1e-12


def test_end_token_position_rule():
    from lightx2v_amd.clip_text import eos_position

    ids = torch.tensor([[5, 9, 3, 9, 0], [7, 7, 7, 7, 7], [1, 2, 40, 2, 40], [3, 4, 5, 6, 8]])
    assert eos_position(ids, 2).tolist() == [1, 0, 2, 4]  # legacy rule: the first position of the largest id (ties: the first)
    assert eos_position(ids, 9).tolist() == [1, 0, 0, 0]  # the first position holding the id; rows without it pool position 0 (argmax of zeros)
    assert eos_position(ids, 40).tolist() == [0, 0, 2, 0]


def test_rope_tables_against_fp64():
    from lightx2v_amd.llama import rope_tables

    cos, sin = rope_tables(500000.0)
    assert cos.shape == sin.shape == (512, 64) and cos.dtype == torch.float32 and cos.is_contiguous()
    pos = torch.arange(512, dtype=torch.float64)[:, None]
    ang = pos * (500000.0 ** (-2.0 * torch.arange(64, dtype=torch.float64) / 128.0))[None]
    assert (cos.double() - ang.cos()).abs().max().item() <= 2.0**-24 and (sin.double() - ang.sin()).abs().max().item() <= 2.0**-24
    assert torch.equal(cos[0], torch.ones(64)) and torch.equal(sin[0], torch.zeros(64))


def test_model_layout_prefixes_and_refusals(llama, clip):
    """Load-time layout (fused q | k | v, the SwiGLU interleave, L - 2 layers), both name prefixes, and every refusal that comes before a launch."""
    from lightx2v_amd import clip_text, lib
    from lightx2v_amd import llama as L

    gold, dims, sd = llama
    m = L.TextEncoderHFLlamaModel((sd, dims), "cpu")
    assert (m.max_length, m.hidden_state_skip_layer, m.crop_start) == (351, 2, 95) and "{}" in m.prompt_template
    assert (m.vocab, m.dim, m.num_heads, m.num_kv_heads, m.dim_ffn, m.num_layers) == (384, 512, 4, 2, 448, 2)
    b = m.blocks[1]
    assert b["qkv"].shape == (1024, 512) and torch.equal(b["qkv"][512:768], sd["layers.1.self_attn.k_proj.weight"])
    assert b["swiglu"].shape == (896, 512)
    assert torch.equal(b["swiglu"][0::2], sd["layers.1.mlp.gate_proj.weight"]) and torch.equal(b["swiglu"][1::2], sd["layers.1.mlp.up_proj.weight"])
    assert m.weight_bytes() == 2 * 2 * (1024 * 512 + 512 * 512 + 3 * 448 * 512) and m.launches() == 14
    assert L.encoder_flops(m, [3]) == 2 * (2 * 3 * (1024 * 512 + 512 * 512 + 3 * 448 * 512) + 4 * 4 * 128 * 6)
    pre = L.TextEncoderHFLlamaModel(({"model." + k: v for k, v in sd.items()}, dims), "cpu")
    assert torch.equal(pre.blocks[0]["o"], m.blocks[0]["o"])
    with pytest.raises(lib.X2VError, match="config gives"):
        L.TextEncoderHFLlamaModel((sd, dict(dims, ffn=480)), "cpu")
    with pytest.raises(lib.X2VError, match="lacks"):
        L.TextEncoderHFLlamaModel(({k: v for k, v in sd.items() if k != "layers.0.mlp.up_proj.weight"}, dims), "cpu")
    with pytest.raises(lib.X2VError, match="head_dim"):
        L.TextEncoderHFLlamaModel((sd, dict(dims, heads=8, kv_heads=4, head_dim=64)), "cpu")
    with pytest.raises(lib.X2VError, match="silu"):
        L.dims_from_config(dict(hidden_act="gelu"))
    cfg = dict(vocab_size=128256, hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, intermediate_size=14336, num_hidden_layers=32, rms_norm_eps=1e-5,
               rope_theta=500000.0, hidden_act="silu")
    from lightx2v_amd import synth

    assert L.dims_from_config(cfg) == synth.LLAMA_DIMS["llama3-8b"]
    ids, mask = gold["ids"][:1], gold["mask"][:1]
    with pytest.raises(lib.X2VError, match="crop_start"):
        m.infer_ids(ids[:, :95], mask[:, :95])
    holed = mask.clone()
    holed[0, 3] = 0
    with pytest.raises(lib.X2VError, match="prefix"):
        m.infer_ids(ids, holed)
    with pytest.raises(lib.X2VError, match="vocabulary"):
        m.infer_ids(ids + 384, mask)
    with pytest.raises(lib.X2VError, match=r"\[1, L\]"):
        m.infer_ids(gold["ids"][:2], gold["mask"][:2])
    with pytest.raises(lib.X2VError, match="pass token ids to infer_ids"):
        m.infer("a cat", None)

    gold, dims, sd = clip
    c = clip_text.TextEncoderHFClipModel((sd, dims), "cpu")
    assert c.max_length == 77 and (c.dim, c.num_heads, c.dim_ffn, c.num_layers, c.eos_token_id) == (256, 4, 2048, 4, 2)
    assert c.blocks[0]["qkv"].shape == (768, 256) and torch.equal(c.blocks[0]["qkv_b"][256:512], sd["text_model.encoder.layers.0.self_attn.k_proj.bias"])
    assert c.final_ln[0].dtype == torch.float32 and c.launches() == 29
    bare = clip_text.TextEncoderHFClipModel(({k[len("text_model."):]: v for k, v in sd.items()}, dims), "cpu")
    assert torch.equal(bare.blocks[1]["fc1"], c.blocks[1]["fc1"])
    with pytest.raises(lib.X2VError, match="config gives"):
        clip_text.TextEncoderHFClipModel((sd, dict(dims, ffn=1024)), "cpu")
    with pytest.raises(lib.X2VError, match="head dim 64"):
        clip_text.TextEncoderHFClipModel((sd, dict(dims, heads=2, head_dim=128)), "cpu")
    with pytest.raises(lib.X2VError, match="quick_gelu"):
        clip_text.dims_from_config(dict(hidden_act="gelu"))
    ids, mask = gold["ids"][2:3], gold["mask"][2:3]
    assert c._pooled_position(ids, mask) == 20
    with pytest.raises(lib.X2VError, match="end token"):
        c.infer_ids(ids, torch.cat([mask[:, :10], torch.zeros(1, 67, dtype=torch.long)], dim=1))
    with pytest.raises(lib.X2VError, match="vocabulary"):
        c.infer_ids(ids + 1, mask)
    with pytest.raises(lib.X2VError, match="pass token ids to infer_ids"):
        c.infer("a cat", None)


def test_plugin_hook_rebinds_the_runner_names(monkeypatch):
    """use_hip_hunyuan_text_encoders swaps the two classes the runner module binds by name and leaves the LLaVA class of i2v alone.  The reference's runner
    module needs packages a test machine may lack, so a stand-in module with the same three names sits at its import path."""
    import sys
    import types

    from lightx2v_amd import clip_text, llama, plugin

    path = "lightx2v.models.runners.hunyuan.hunyuan_runner"
    parts = path.split(".")
    for i in range(1, len(parts) + 1):
        mod = types.ModuleType(".".join(parts[:i]))
        mod.__path__ = []
        monkeypatch.setitem(sys.modules, mod.__name__, mod)
    runner = sys.modules[path]
    runner.TextEncoderHFLlamaModel = runner.TextEncoderHFClipModel = runner.TextEncoderHFLlavaModel = object
    sys.modules["lightx2v.models.runners.hunyuan"].hunyuan_runner = runner
    plugin.use_hip_hunyuan_text_encoders()
    assert runner.TextEncoderHFLlamaModel is llama.TextEncoderHFLlamaModel and runner.TextEncoderHFClipModel is clip_text.TextEncoderHFClipModel
    assert runner.TextEncoderHFLlavaModel is object


def test_new_entries_validate_arguments_without_a_gpu():
    from lightx2v_amd import lib

    L = lib._lib
    a = ctypes.c_void_p(4096)
    cu = (ctypes.c_int * 3)(0, 5, 9)
    # x2v_attn_f16_causal(qkv, ld, out, ldo, cu_seqlens, batch, num_heads, num_kv_heads, head_dim, rope_cos, rope_sin, scale, stream)
    assert L.x2v_attn_f16_causal(None, 1024, a, 512, cu, 2, 4, 2, 128, None, None, 0.0, None) == -5
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, cu, 2, 4, 2, 80, None, None, 0.0, None) == -1  # head_dim
    assert b"head_dim=80" in L.x2v_last_error()
    assert L.x2v_attn_f16_causal(a, 384, a, 128, cu, 2, 2, 2, 64, a, a, 0.0, None) == -5  # rope tables with head_dim 64
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, cu, 2, 4, 2, 128, a, None, 0.0, None) == -5  # one table only
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, cu, 2, 4, 3, 128, None, None, 0.0, None) == -1  # 4 % 3
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, cu, 9, 4, 2, 128, None, None, 0.0, None) == -1  # batch
    assert L.x2v_attn_f16_causal(a, 1016, a, 512, cu, 2, 4, 2, 128, None, None, 0.0, None) == -2  # ld does not cover q | k | v
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, (ctypes.c_int * 3)(0, 5, 5), 2, 4, 2, 128, None, None, 0.0, None) == -1  # an empty sequence
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, (ctypes.c_int * 2)(0, 513), 1, 4, 2, 128, None, None, 0.0, None) == -1  # > 512 tokens
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, (ctypes.c_int * 2)(-1, 8), 1, 4, 2, 128, None, None, 0.0, None) == -1  # negative cu_seqlens[0]
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, (ctypes.c_int * 3)(0, 8, 5), 2, 4, 2, 128, None, None, 0.0, None) == -1  # decreasing
    assert L.x2v_attn_f16_causal(a, 1024, a, 512, cu, 2, 4, 2, 128, None, None, -1.0, None) == -5  # negative scale
    # x2v_gemm_f16(x, ldx, w, ldw, bias, y, ldy, M, N, K, epilogue, resid, ldr, stream)
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 4, 64, 64, 5, None, 0, None) == -5  # unknown epilogue
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 4, 64, 64, 3, None, 0, None) == -5  # quick-GELU without a bias
    assert b"quick-GELU" in L.x2v_last_error()
    assert L.x2v_gemm_f16(a, 64, a, 64, a, a, 64, 4, 64, 64, 4, None, 0, None) == -5  # SwiGLU with a bias
    assert b"SwiGLU" in L.x2v_last_error()
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 4, 63, 64, 4, None, 0, None) == -1  # SwiGLU with odd N
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 60, 4, 64, 64, 4, None, 0, None) == -2  # ldy < N
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 0, 64, 64, 4, None, 0, None) == 0  # no rows: nothing launched
    assert L.x2v_gemm_f16(a, 64, a, 64, a, a, 64, 0, 64, 64, 3, None, 0, None) == 0
    # x2v_rmsnorm_f16(x, ldx, w, y, ldy, M, D, eps, stream)
    assert L.x2v_rmsnorm_f16(a, 16, None, a, 16, 1, 16, 1e-5, None) == -5
    assert L.x2v_rmsnorm_f16(a, 16, a, a, 16, 1, 12, 1e-5, None) == -1
    assert L.x2v_rmsnorm_f16(a, 8200, a, a, 8200, 1, 8200, 1e-5, None) == -1  # D > 8192
    assert L.x2v_rmsnorm_f16(a, 8, a, a, 16, 1, 16, 1e-5, None) == -2  # ldx < D
    assert L.x2v_rmsnorm_f16(a, 16, a, a, 16, 0, 16, 1e-5, None) == 0
