"""Host-side checks of the quantised umT5 encoder path (no GPU): quantize_state_dict's layout, the constructor's fused / interleaved weights and scales, its
refusals, and the quantised restatement's two evaluations against each other."""
import pytest
import torch

SCHEMES = {"int8": (torch.int8, 127.0), "fp8": (torch.float8_e4m3fn, 448.0)}
LINEARS = ("attn.q", "attn.k", "attn.v", "attn.o", "ffn.fc1", "ffn.gate.0", "ffn.fc2")


@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("t5_encoder_tiny")


@pytest.fixture(scope="module")
def tiny_sd(gold):
    from lightx2v_amd import synth

    return synth.synth_t5_weights(synth.T5_DIMS["t5-tiny"], seed=int(gold["seed"][0]))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_quantize_state_dict_layout_and_model_rows(tiny_sd, scheme):
    """The reference's layout (codes [N, K], weight_scale [N, 1] fp32 = max(amax, 1e-5) / qmax, everything else bf16), dequantising to within half a step of
    each channel (e4m3: half of its widest spacing, 32 code units below 448); and the constructor's fused q | k | v and interleaved fc1 / gate.0 rows, scales alongside."""
    from lightx2v_amd import t5

    dtype, qmax = SCHEMES[scheme]
    qsd = t5.quantize_state_dict(tiny_sd, scheme)
    assert set(qsd) == set(tiny_sd) | {f"blocks.{i}.{n}.weight_scale" for i in range(2) for n in LINEARS}
    for k, v in tiny_sd.items():
        if k.split(".")[-2] not in ("q", "k", "v", "o", "fc1", "0", "fc2"):
            assert torch.equal(qsd[k], v)
            continue
        q, s = qsd[k], qsd[k + "_scale"]
        assert q.dtype == dtype and q.shape == v.shape and s.dtype == torch.float32 and s.shape == (v.shape[0], 1)
        assert torch.equal(s, v.float().abs().amax(dim=1, keepdim=True).clamp(min=1e-5) / qmax)
        assert ((q.float() * s - v.float()).abs() <= ((0.5 if scheme == "int8" else 16.0) + qmax * 2.0**-23) * s).all()  # + the fp32 rounding of w / s
    m = t5.T5EncoderModel(512, torch.bfloat16, "cpu", None, t5_quantized=True, t5_quantized_ckpt=qsd, quant_scheme=scheme)
    b, p = m.blocks[1], "blocks.1."
    assert b["qkv"].dtype == dtype and b["qkv"].shape == (768, 256) and b["qkv_s"].shape == (768,) and b["geglu"].shape == (1280, 256) and b["geglu_s"].shape == (1280,)
    for row, name, src in ((5, "qkv", "attn.q"), (256 + 7, "qkv", "attn.k"), (2 * 9, "geglu", "ffn.fc1"), (2 * 9 + 1, "geglu", "ffn.gate.0")):
        n = {"attn.q": 5, "attn.k": 7}.get(src, 9)
        assert torch.equal(b[name][row].view(torch.uint8), qsd[p + src + ".weight"][n].view(torch.uint8)) and b[name + "_s"][row] == qsd[p + src + ".weight_scale"][n, 0]
    assert 2 * m.weight_bytes() == t5.T5EncoderModel(512, torch.bfloat16, "cpu", tiny_sd).weight_bytes()
    assert {k: v.dtype for k, v in m._workspace(5).items()}["codes"] == torch.uint8 and "h" not in m._bufs


def test_constructor_refusals(tiny_sd):
    from lightx2v_amd import lib, t5

    q8 = t5.quantize_state_dict(tiny_sd, "int8")
    with pytest.raises(lib.X2VError, match="quant_scheme"):
        t5.T5EncoderModel(512, torch.bfloat16, "cpu", None, t5_quantized=True, t5_quantized_ckpt=q8, quant_scheme="int4")
    with pytest.raises(lib.X2VError, match="quant_scheme"):
        t5.quantize_state_dict(tiny_sd, "nf4")
    with pytest.raises(lib.X2VError, match="torch.int8"):
        t5.T5EncoderModel(512, torch.bfloat16, "cpu", None, t5_quantized=True, t5_quantized_ckpt=q8, quant_scheme="fp8")
    with pytest.raises(lib.X2VError, match="weight_scale"):
        t5.T5EncoderModel(512, torch.bfloat16, "cpu", None, t5_quantized=True, quant_scheme="int8",
                          t5_quantized_ckpt={k: v for k, v in q8.items() if k != "blocks.1.ffn.fc2.weight_scale"})
    with pytest.raises(NotImplementedError, match="t5_quantized_ckpt"):
        t5.T5EncoderModel(512, torch.bfloat16, "cpu", tiny_sd, t5_quantized=True, quant_scheme="int8")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_restatement_bf16_order_against_fp64(gold, tiny_sd, scheme):
    """The sanity anchor of the GPU test's truth.  The unquantised encoder's bf16 evaluation sits e0 from its fp64 one.  Between two evaluations of the
    quantised encoder that noise also moves activations across code boundaries, and a re-drawn code is a fresh draw of the quantisation noise, whose size is
    eq = err(quantised fp64 vs unquantised fp64): the two quantised evaluations must agree to e0 + eq (CPU: int8 2.6e-2 of 3.5e-2, fp8 6.4e-2 of 9.4e-2 at
    worst), and the fp32 evaluation, which only re-draws a code at an exact tie, lies closer to the truth than the bf16 one."""
    from lightx2v_amd import t5
    from tests import t5_quant_restatement as Q
    from tests import t5_restatement as R
    from tests.test_gpu_t5 import _rel

    qsd = t5.quantize_state_dict(tiny_sd, scheme)
    args = (gold["ids"], gold["mask"])
    plain64, plain16 = (R.infer_ids(tiny_sd, *args, dtype=d) for d in (torch.float64, torch.bfloat16))
    q64, q32, q16 = (Q.infer_ids(qsd, *args, scheme, dtype=d) for d in (torch.float64, torch.float32, torch.bfloat16))
    for b in range(4):
        e0, eq, e16, e32 = _rel(plain16[b], plain64[b]), _rel(q64[b], plain64[b]), _rel(q16[b], q64[b]), _rel(q32[b], q64[b])
        print(f"{scheme} prompt {b}: bf16 vs fp64 {e16:.3e} (unquantised {e0:.3e}, quantisation {eq:.3e}), fp32 vs fp64 {e32:.3e}")
        assert q16[b].dtype == torch.bfloat16 and e16 <= e0 + eq and e32 <= e16
