"""CLIP image tower, host side (no GPU): the plain-PyTorch restatement against the reference fixture, the public interface against the reference's,
the synthetic checkpoint's key set, the fp16 range of a synthetic 31-block forward, and the new C-ABI entries' argument checks.

Bit-exactness: the restatement reproduces the reference's outputs bit for bit in the fp32 model AND in the fp16 model on the CPU (same torch functions
on the same dtypes and layouts as the module under CPU autocast), so both are asserted with torch.equal."""
import ctypes
import inspect

import pytest
import torch

from lightx2v_amd import lib, synth
from tests import clip_restatement as R
from tests.util import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("clip_visual_tiny")


def _sd(gold):
    sd = synth.synth_clip_weights(synth.CLIP_DIMS["clip-tiny"], seed=int(gold["seed"][0]))
    checksum = sum((sd[k].double().abs().sum() for k in sorted(sd)), torch.zeros((), dtype=torch.float64)).reshape(1)  # oracle/gen_golden.py::weights_checksum
    assert torch.equal(checksum, gold["weights_checksum"]), "synth_clip_weights drifted from the fixture"
    return sd


def test_restatement_preprocess_matches_reference_fixture(gold):
    """The fixture's `preprocessed` tensor is the generator's own F.interpolate + stand-in Normalize (tools/gen_golden_clip.py), not a tensor taken out
    of the reference's visual(): this guards the restatement's front end against drift; the reference's is pinned through the out_* tensors below."""
    pre =R.preprocess([gold["image_a"], gold["image_b"]])
    assert torch.equal(pre, gold["preprocessed"])
    # 224 x 224 input: the bicubic resize is the identity
    b = gold["image_b"][:, 0]
    m, s = torch.tensor(synth.CLIP_MEAN).view(3, 1, 1), torch.tensor(synth.CLIP_STD).view(3, 1, 1)
    assert torch.equal(pre[1], (b * 0.5 + 0.5 - m) / s)


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("tag, dtype", [("f32", torch.float32), ("f16", torch.float16)])
def test_restatement_matches_reference_fixture(gold, name, tag, dtype):
    sd = _sd(gold)
    out = R.visual(sd, [gold[f"image_{name}"]], dtype=dtype)
    ref = gold[f"out_{tag}_{name}"]
    assert out.shape == ref.shape == (1, 257, 160) and out.dtype == ref.dtype == dtype
    assert torch.equal(out, ref), f"max |d| {(out.float() - ref.float()).abs().max().item():.3e}"


def test_fixture_fp16_error_is_an_fp16_error(gold):
    """The yardstick of the GPU triangle test: the reference's own fp16-vs-fp32 relative L2 on the fixture is that of fp16 arithmetic (1e-4 .. 3e-3)."""
    for name in "ab":
        e = ((gold[f"out_f16_{name}"].float() - gold[f"out_f32_{name}"]).norm() / gold[f"out_f32_{name}"].norm()).item()
        assert 1e-4 < e < 3e-3, e


def test_synth_clip_weights_shapes_and_released_dims():
    d = synth.CLIP_DIMS["clip-vit-h-14"]
    assert (d["dim"], d["heads"], d["layers"], d["patch_size"], d["image_size"]) == (1280, 16, 32, 14, 224)
    t = synth.CLIP_DIMS["clip-tiny"]
    assert t["dim"] // t["heads"] == 80 and t["patch_size"] == 14 and t["layers"] == 3
    sd = synth.synth_clip_weights(t, seed=1)
    assert sd["visual.patch_embedding.weight"].shape == (160, 3, 14, 14) and sd["visual.pos_embedding"].shape == (1, 257, 160)
    assert sd["visual.transformer.2.attn.to_qkv.weight"].shape == (480, 160) and sd["visual.transformer.0.mlp.2.weight"].shape == (160, 640)
    assert sd["visual.cls_embedding"].shape == (1, 1, 160) and sd["visual.head"].shape == (160, 1024) and "visual.transformer.3.norm1.weight" not in sd
    assert all(v.dtype == torch.float16 for k, v in sd.items() if k != "log_scale")
    # synth_i2v_inputs is untouched by the new stream
    assert synth.synth_i2v_inputs(synth.WAN_DIMS["wan-tiny-i2v"], (16, 3, 8, 8))["clip_encoder_out"].shape == (257, 64)


def test_synth_31_block_forward_stays_far_from_the_fp16_range():
    """A 31-block tower at 2 heads x 80 with synth_clip_weights' scaling, run by the restatement in fp32 on the CPU: the residual stream and the widest
    intermediate (the MLP's hidden layer is bounded by the same Linear scaling) stay below 1e3, two orders under fp16's 65504."""
    dims = dict(synth.CLIP_DIMS["clip-tiny"], layers=32)
    sd = synth.synth_clip_weights(dims, seed=2)
    img = torch.rand(3, 1, 64, 80, generator=torch.Generator().manual_seed(1)) * 2 - 1
    out = R.visual(sd, [img])
    assert out.shape == (1, 257, 160) and torch.isfinite(out).all()
    assert out.abs().max().item() < 1e3


def _reference_clip():
    """The unmodified reference's CLIP module.  Whether to skip is decided before any work (no reference checkout, or no `transformers`, which the
    module imports); everything after that runs unguarded, so a broken tool, stand-in or reference import fails the test."""
    from oracle import ref_import

    if not ref_import.reference_available():
        pytest.skip("reference checkout not present")
    pytest.importorskip("transformers")
    from tools.gen_golden_clip import import_reference_clip

    return import_reference_clip()


def test_interface_matches_reference():
    from lightx2v_amd import clip

    ref = _reference_clip()
    for name in ("__init__", "visual", "to_cuda", "to_cpu"):
        assert list(inspect.signature(getattr(clip.CLIPModel, name)).parameters) == list(inspect.signature(getattr(ref.CLIPModel, name)).parameters), name


def test_synth_keys_equal_reference_state_dict():
    ref = _reference_clip()
    for name in ("clip-tiny",):
        d = synth.CLIP_DIMS[name]
        m = ref.clip_xlm_roberta_vit_h_14(pretrained=False, dtype=torch.float16, device="cpu", vision_dim=d["dim"], vision_heads=d["heads"], vision_layers=d["layers"])
        want = {k: tuple(v.shape) for k, v in m.state_dict().items() if "textual" not in k}
        got = {k: tuple(v.shape) for k, v in synth.synth_clip_weights(d).items()}
        assert got == want


def test_plugin_binds_the_name_the_runner_resolves(tmp_path, monkeypatch):
    """plugin.use_hip_clip_encoder() against the reference's runner source.  runners/wan/wan_runner.py cannot be imported on a host without a GPU (the
    T5 module it imports evaluates torch.cuda.current_device() in a default argument, and the runner needs imageio), so its text is parsed instead: the
    module binds the class under the module-level name `CLIPModel`, `load_image_encoder` calls that name with keywords only, and exactly those
    keywords, with the runner's values for an unquantised config, construct this package's class from a .pth checkpoint.  The rebinding itself is run on
    a stand-in module object placed under the runner's module name (removed again by monkeypatch)."""
    import ast
    import os
    import sys
    import types

    from lightx2v_amd import clip, plugin
    from oracle import ref_import

    if not ref_import.reference_available():
        pytest.skip("reference checkout not present")
    ref_import.patch_and_import()
    path = os.path.join(ref_import.REFERENCE_ROOT, "lightx2v", "models", "runners", "wan", "wan_runner.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    imported = [(n.module, a.asname or a.name) for n in tree.body if isinstance(n, ast.ImportFrom) for a in n.names if a.name == "CLIPModel"]
    assert imported == [("lightx2v.models.input_encoders.hf.xlm_roberta.model", "CLIPModel")]
    load = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "load_image_encoder")
    calls = [n for n in ast.walk(load) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "CLIPModel"]
    assert len(calls) == 1 and not calls[0].args
    keywords = [k.arg for k in calls[0].keywords]
    assert keywords == ["dtype", "device", "checkpoint_path", "clip_quantized", "clip_quantized_ckpt", "quant_scheme"]

    name = "lightx2v.models.runners.wan.wan_runner"
    stand_in = types.ModuleType(name)
    stand_in.CLIPModel = object
    monkeypatch.setitem(sys.modules, name, stand_in)
    plugin.use_hip_clip_encoder()
    assert stand_in.CLIPModel is clip.CLIPModel

    ckpt = tmp_path / "models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth"
    torch.save(synth.synth_clip_weights(synth.CLIP_DIMS["clip-tiny"]), str(ckpt))
    values = dict(dtype=torch.float16, device=torch.device("cpu"), checkpoint_path=str(ckpt), clip_quantized=False, clip_quantized_ckpt=None, quant_scheme=None)  # wan_runner.py:56-81
    m = stand_in.CLIPModel(**{k: values[k] for k in keywords})
    assert (m.dim, m.num_heads, len(m.blocks)) == (160, 2, 2) and callable(m.visual)
    with pytest.raises(NotImplementedError, match="clip_quantized"):
        stand_in.CLIPModel(**dict(values, clip_quantized=True, clip_quantized_ckpt="clip-fp8.pth", quant_scheme="fp8"))


def test_clip_model_refusals_need_no_gpu():
    from lightx2v_amd import clip

    sd = synth.synth_clip_weights(synth.CLIP_DIMS["clip-tiny"])
    with pytest.raises(NotImplementedError, match="clip_quantized"):
        clip.CLIPModel(torch.float16, "cpu", sd, True, None, "fp8")
    with pytest.raises(lib.X2VError, match="fp16"):
        clip.CLIPModel(torch.bfloat16, "cpu", sd, False, None, None)
    with pytest.raises(lib.X2VError, match="lacks"):
        clip.CLIPModel(torch.float16, "cpu", {k: v for k, v in sd.items() if "pos_embedding" not in k}, False, None, None)
    sd["textual.token_embedding.weight"] = torch.zeros(4, 4)  # ignored (model.py:428-430)
    m = clip.CLIPModel(torch.float16, "cpu", sd, False, None, None)
    assert (m.dim, m.num_heads, m.num_layers, m.tokens, m.image_size, m.patch_size, m.k_pad, len(m.blocks)) == (160, 2, 3, 257, 224, 14, 608, 2)
    assert m.pre_norm[0].dtype == torch.float32 and m.blocks[0]["n1"][1].dtype == torch.float32 and m.w_patch.shape == (160, 608) and not m.w_patch[:, 588:].any()
    with pytest.raises(lib.X2VError):  # no CPU fallback
        m.visual([torch.zeros(3, 1, 32, 32)], None)


def test_gemm_f16_tile_choice_is_host_arithmetic():
    assert lib.gemm_f16_tile_choice(257, 3840) == (64, 64) and lib.gemm_f16_tile_choice(257, 5120) == (128, 64)
    assert lib.gemm_f16_tile_choice(257, 1280) == (64, 32) and lib.gemm_f16_tile_choice(1028, 1280) == (64, 64) and lib.gemm_f16_tile_choice(1028, 3840) == (128, 64) and lib.gemm_f16_tile_choice(257, 160) == (64, 16)


def test_clip_abi_argument_validation_needs_no_gpu():
    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)
    # x2v_gemm_f16(x, ldx, w, ldw, bias, y, ldy, M, N, K, epilogue, resid, ldr, stream)
    assert L.x2v_gemm_f16(None, 64, a, 64, None, a, 64, 4, 64, 64, 0, None, 0, None) == -5
    assert L.x2v_gemm_f16(a, 600, a, 600, None, a, 64, 4, 64, 588, 0, None, 0, None) == -1  # K % 32
    assert b"K=588" in L.x2v_last_error()
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 4, 62, 64, 0, None, 0, None) == -1  # N % 4
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 4, 64, 64, 3, None, 0, None) == -5  # unknown epilogue
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 4, 64, 64, 2, None, 0, None) == -5  # residual epilogue without resid
    assert L.x2v_gemm_f16(a, 60, a, 64, None, a, 64, 4, 64, 64, 0, None, 0, None) == -2  # ldx < K
    assert L.x2v_gemm_f16(odd, 64, a, 64, None, a, 64, 4, 64, 64, 0, None, 0, None) == -2  # alignment
    assert L.x2v_gemm_f16(a, 64, a, 64, None, a, 64, 0, 64, 64, 0, None, 0, None) == 0  # no rows: nothing launched
    assert L.x2v_gemm_f16_tile_choice(0, 64) == -1
    # x2v_attn_f16_d80(qkv, ld, out, ldo, batch, S, heads, scale, stream)
    assert L.x2v_attn_f16_d80(None, 3840, a, 1280, 1, 257, 16, 0.0, None) == -5
    assert L.x2v_attn_f16_d80(a, 3840, a, 1280, 1, 273, 16, 0.0, None) == -1  # more keys than the LDS image holds
    assert b"S=273" in L.x2v_last_error()
    assert L.x2v_attn_f16_d80(a, 3840, a, 1280, 0, 257, 16, 0.0, None) == -1
    assert L.x2v_attn_f16_d80(a, 3832, a, 1280, 1, 257, 16, 0.0, None) == -2  # ld below 3 * 16 * 80
    assert L.x2v_attn_f16_d80(a, 3840, odd, 1280, 1, 257, 16, 0.0, None) == -2
    # x2v_layernorm_f16(x, ldx, w, b, y, ldy, M, D, eps, stream)
    assert L.x2v_layernorm_f16(a, 1280, None, a, a, 1280, 4, 1280, 1e-5, None) == -5
    assert L.x2v_layernorm_f16(a, 1284, a, a, a, 1284, 4, 1284, 1e-5, None) == -1  # D % 8
    assert L.x2v_layernorm_f16(a, 4096, a, a, a, 4096, 4, 4096, 1e-5, None) == -1  # D > 2048
    assert L.x2v_layernorm_f16(a, 1272, a, a, a, 1280, 4, 1280, 1e-5, None) == -2
    assert L.x2v_layernorm_f16(a, 1280, a, a, a, 1280, 0, 1280, 1e-5, None) == 0
    # x2v_clip_embed_f16(patches, ldp, cls, pos, w, b, y, ldy, batch, tokens, D, eps, stream)
    assert L.x2v_clip_embed_f16(a, 1280, None, a, a, a, a, 1280, 1, 257, 1280, 1e-5, None) == -5
    assert L.x2v_clip_embed_f16(a, 1280, a, a, a, a, a, 1280, 1, 1, 1280, 1e-5, None) == -1  # no patch tokens
    assert L.x2v_clip_embed_f16(a, 1280, a, a, a, a, a, 1276, 1, 257, 1280, 1e-5, None) == -2
    # x2v_clip_preprocess_f16(img, cs, rs, H, W, out, ld_out, image_size, patch, mean x 3, std x 3, stream)
    ms = (0.5, 0.5, 0.5, 0.25, 0.25, 0.25)
    assert L.x2v_clip_preprocess_f16(None, 64, 8, 8, 8, a, 608, 224, 14, *ms, None) == -5
    assert L.x2v_clip_preprocess_f16(a, 64, 8, 8, 8, a, 608, 220, 14, *ms, None) == -1  # image_size % patch
    assert L.x2v_clip_preprocess_f16(a, 64, 8, 8, 8, a, 584, 224, 14, *ms, None) == -1  # ld_out < 3 * 14 * 14
    assert L.x2v_clip_preprocess_f16(a, 60, 8, 8, 8, a, 608, 224, 14, *ms, None) == -1  # channel stride below the image
    assert L.x2v_clip_preprocess_f16(a, 64, 8, 8, 8, a, 608, 224, 14, 0.5, 0.5, 0.5, 0.25, 0.0, 0.25, None) == -5  # zero std
    assert L.x2v_clip_preprocess_f16(a, 64, 8, 8, 8, ctypes.c_void_p(4098), 608, 224, 14, *ms, None) == -2
