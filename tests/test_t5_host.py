"""Host-side checks of the umT5 text encoder path (no GPU): the restatement (tests/t5_restatement.py) against the fixture generated from the unmodified
reference (tests/golden/t5_encoder_tiny.*.safetensors, tools/gen_golden_t5.py) and, where the reference checkout is present, against the live reference; the
host bucket function; the synthetic checkpoint's names; the argument that lets the HIP path run on the valid tokens only; the constructor's refusals and the
C entries' argument validation (before any HIP call)."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("t5_encoder_tiny")


@pytest.fixture(scope="module")
def tiny_sd(gold):
    from lightx2v_amd import synth

    return synth.synth_t5_weights(synth.T5_DIMS["t5-tiny"], seed=int(gold["seed"][0]))


def test_synth_weights_match_the_fixture_checksum(gold, tiny_sd):
    from oracle.gen_golden import weights_checksum

    assert torch.equal(weights_checksum(tiny_sd), gold["weights_checksum"])
    assert all(v.dtype == torch.bfloat16 for v in tiny_sd.values())


def test_restatement_bf16_equals_the_reference_fixture_bit_for_bit(gold, tiny_sd):
    from tests import t5_restatement as R

    assert [int(n) for n in gold["mask"].sum(dim=1)] == [37, 64, 1, 130]
    full = R.encoder(tiny_sd, gold["ids"], gold["mask"], dtype=torch.bfloat16)
    assert full.dtype == torch.bfloat16 and torch.equal(full, gold["out_padded"])
    outs = R.infer_ids(tiny_sd, gold["ids"], gold["mask"], dtype=torch.bfloat16)
    for b, o in enumerate(outs):
        assert torch.equal(o, gold[f"out_{b}"]), f"prompt {b}"


def test_host_bucket_function_equals_the_reference_vector(gold):
    """The delta → bucket map the bias tables are built from, for every delta a 512-token prompt has; the map is not symmetric in the delta."""
    from lightx2v_amd import t5

    b = t5.relative_position_bucket(torch.arange(-511, 512))
    assert torch.equal(b, gold["buckets"])
    assert b[511] == 0 and b[511 + 1] == 17 and b[511 - 1] == 1 and int(b.max()) == 31
    emb = torch.randn(32, 4, generator=torch.Generator().manual_seed(0))
    tab = t5.bias_table(emb)
    assert tab.shape == (4, 1023) and tab.dtype == torch.float32
    assert torch.equal(tab[:, 511 + 3], emb[16 + 3]) and torch.equal(tab[:, 511 - 3], emb[3])


@pytest.fixture
def live_reference():
    """(tools/gen_golden_t5 module, the reference's t5 model module), with the stand-ins the import needs (empty `ftfy` / `vllm` modules in sys.modules,
    torch.cuda.current_device) taken back afterwards: no later test sees them."""
    import importlib.util
    import os
    import sys

    from oracle import ref_import

    if not ref_import.reference_available():
        pytest.skip("the reference checkout is not on this machine")
    names = ("ftfy", "vllm", "vllm._custom_ops")
    before, current_device = {n: sys.modules.get(n) for n in names}, torch.cuda.current_device
    spec = importlib.util.spec_from_file_location("gen_golden_t5", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_golden_t5.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    try:
        yield tool, tool.import_reference_t5()
    finally:
        torch.cuda.current_device = current_device
        for n, mod in before.items():
            if mod is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = mod


def test_synth_state_dict_names_equal_the_live_reference(live_reference):
    from lightx2v_amd import synth

    tool, ref = live_reference
    dims = synth.T5_DIMS["t5-tiny"]
    sd = synth.synth_t5_weights(dims, seed=1)
    want = tool.build_reference(ref, sd, dims).state_dict()
    assert set(sd) == set(want)
    assert all(tuple(sd[k].shape) == tuple(want[k].shape) for k in sd)


def test_restatement_bf16_equals_the_live_reference_on_another_seed(live_reference):
    from lightx2v_amd import synth
    from tests import t5_restatement as R

    tool, ref = live_reference
    dims = synth.T5_DIMS["t5-tiny"]
    sd = synth.synth_t5_weights(dims, seed=9)
    ids, mask = tool.make_ids((5, 96, 33), 96, dims["vocab"], 3)
    with torch.no_grad():
        want = tool.build_reference(ref, sd, dims)(ids, mask)
    assert torch.equal(R.encoder(sd, ids, mask, dtype=torch.bfloat16), want)


def test_valid_rows_do_not_depend_on_padding(gold, tiny_sd):
    """The packing argument: padded keys get probability exactly 0, so the fp64 restatement on a prompt's valid tokens alone equals its valid rows in the
    padded batch (1e-12: summation order inside torch only)."""
    from tests import t5_restatement as R

    ids, mask = gold["ids"], gold["mask"]
    padded = R.infer_ids(tiny_sd, ids, mask, dtype=torch.float64)
    for b, n in enumerate(int(n) for n in mask.sum(dim=1)):
        alone = R.encoder(tiny_sd, ids[b : b + 1, :n], mask[b : b + 1, :n], dtype=torch.float64)[0]
        d = (alone - padded[b]).abs().max().item()
        assert d <= 1e-12 * max(1.0, padded[b].abs().max().item()), f"prompt {b}: {d:.3e}"


def test_constructor_refusals(tiny_sd):
    from lightx2v_amd import lib, t5

    with pytest.raises(NotImplementedError, match="t5_quantized"):
        t5.T5EncoderModel(512, torch.bfloat16, "cpu", tiny_sd, t5_quantized=True, quant_scheme="int8")
    with pytest.raises(lib.X2VError, match="bf16"):
        t5.T5EncoderModel(512, torch.float16, "cpu", tiny_sd)
    wide = dict(tiny_sd)
    for i in range(2):
        wide[f"blocks.{i}.pos_embedding.embedding.weight"] = torch.zeros(32, 2, dtype=torch.bfloat16)  # 256 / 2 heads: head dim 128
    with pytest.raises(lib.X2VError, match="head dim 64"):
        t5.T5EncoderModel(512, torch.bfloat16, "cpu", wide)
    with pytest.raises(lib.X2VError, match="lacks"):
        t5.T5EncoderModel(512, torch.bfloat16, "cpu", {k: v for k, v in tiny_sd.items() if k != "norm.weight"})


def test_model_layout_and_id_checks_need_no_gpu(tiny_sd):
    """The load-time layout (fused q | k | v, interleaved fc1 / gate.0, per-block bias tables) and infer_ids' refusals, which come before any launch."""
    from lightx2v_amd import lib, t5

    m = t5.T5EncoderModel(512, torch.bfloat16, "cpu", tiny_sd)
    assert (m.vocab, m.dim, m.dim_attn, m.dim_ffn, m.num_heads, m.num_layers, m.num_buckets) == (384, 256, 256, 640, 4, 2, 32)
    b = m.blocks[1]
    assert b["qkv"].shape == (768, 256) and torch.equal(b["qkv"][256:512], tiny_sd["blocks.1.attn.k.weight"])
    assert b["geglu"].shape == (1280, 256)
    assert torch.equal(b["geglu"][0::2], tiny_sd["blocks.1.ffn.fc1.weight"]) and torch.equal(b["geglu"][1::2], tiny_sd["blocks.1.ffn.gate.0.weight"])
    emb = tiny_sd["blocks.1.pos_embedding.embedding.weight"].float()
    assert b["bias"].shape == (4, 1023) and torch.equal(b["bias"][:, 511 + 200], emb[31]) and torch.equal(b["bias"][:, 511 - 200], emb[15])
    assert m.weight_bytes() == 2 * 2 * (4 * 256 * 256 + 3 * 256 * 640)
    assert t5.encoder_flops(m, [3, 5]) == 2 * (2 * 8 * (4 * 256 * 256 + 3 * 256 * 640) + 4 * 4 * 64 * (9 + 25))
    ids, mask = torch.ones(2, 8, dtype=torch.long), torch.ones(2, 8, dtype=torch.long)
    mask[1] = 0
    with pytest.raises(lib.X2VError, match="no valid token"):
        m.infer_ids(ids, mask)
    mask[1] = torch.tensor([1, 0, 1, 0, 0, 0, 0, 0])
    with pytest.raises(lib.X2VError, match="prefix"):
        m.infer_ids(ids, mask)
    with pytest.raises(lib.X2VError, match="at most 8 prompts"):
        m.infer_ids(torch.ones(9, 8, dtype=torch.long), torch.ones(9, 8, dtype=torch.long))
    with pytest.raises(lib.X2VError, match="at most 512 tokens"):
        m.infer_ids(torch.ones(1, 513, dtype=torch.long), torch.ones(1, 513, dtype=torch.long))
    with pytest.raises(lib.X2VError, match="vocabulary"):
        m.infer_ids(torch.full((1, 4), 384), torch.ones(1, 4, dtype=torch.long))
    m.tokenizer_path = "/nonexistent/tokenizer"
    try:
        import ftfy  # noqa: F401

        missing = "no tokenizer could be loaded"
    except ImportError:
        missing = "`ftfy` package"
    with pytest.raises(lib.X2VError, match=missing):  # which of the two is reported depends on the machine alone, not on test order
        m.infer(["a prompt"])


def test_one_workspace_and_a_bounded_plan_cache(tiny_sd):
    """The model holds ONE workspace, sized to the largest M seen (smaller passes are row views of it), and at most MAX_PLANS launch plans: encoding
    prompts of many different lengths does not grow device memory with the number of lengths."""
    from lightx2v_amd import t5

    m = t5.T5EncoderModel(512, torch.bfloat16, "cpu", tiny_sd)
    a = m._workspace(40)
    b = m._workspace(7)
    assert all(b[k].data_ptr() == a[k].data_ptr() and b[k].shape[0] == 7 for k in a) and m._rows == 40
    for n in range(1, t5.MAX_PLANS + 6):
        m._plan((n,), None)
    assert len(m._plans) == t5.MAX_PLANS and (1,) not in [k[0] for k in m._plans] and m._rows == 40
    m._plan((3, 60), None)  # M = 63 > 40: the workspace grows, and the plans that held its pointers go
    assert m._rows == 63 and list(m._plans) == [((3, 60), None)]
    assert sum(v.numel() * 2 for v in m._bufs.values()) == 63 * 2 * (3 * 256 + 3 * 256 + 256 + 640)


def test_argument_validation_needs_no_gpu():
    """x2v_gemm_rows_bf16 / x2v_attn_bf16_d64_relbias answer their X2V_E_* code, with the entry's name in x2v_last_error(), before any HIP call."""
    from lightx2v_amd import lib

    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)

    def err(rc, code, name):
        assert rc == code, (rc, L.x2v_last_error())
        assert name in L.x2v_last_error(), L.x2v_last_error()

    # x2v_gemm_rows_bf16(x, ldx, w, ldw, y, ldy, M, N, K, epilogue, resid, ldr, stream)
    g = b"gemm_rows_bf16"
    err(L.x2v_gemm_rows_bf16(None, 64, a, 64, a, 64, 4, 64, 64, 0, None, 0, None), -5, g)  # null
    err(L.x2v_gemm_rows_bf16(a, 80, a, 80, a, 64, 4, 64, 80, 0, None, 0, None), -1, g)  # K % 32
    assert b"K=80" in L.x2v_last_error()
    err(L.x2v_gemm_rows_bf16(a, 64, a, 64, a, 64, 4, 62, 64, 0, None, 0, None), -1, g)  # N % 4
    err(L.x2v_gemm_rows_bf16(a, 64, a, 64, a, 64, 4, 64, 64, 1, None, 0, None), -5, g)  # 1 is the fp16 entry's GELU: unknown here
    err(L.x2v_gemm_rows_bf16(a, 64, a, 64, a, 64, 4, 64, 64, 2, None, 0, None), -5, g)  # residual epilogue without resid
    err(L.x2v_gemm_rows_bf16(a, 64, a, 64, a, 64, 4, 64, 64, 3, a, 64, None), -5, g)  # resid with GEGLU
    err(L.x2v_gemm_rows_bf16(a, 64, a, 64, a, 64, 4097, 64, 64, 0, None, 0, None), -1, g)  # M beyond the small-M form
    err(L.x2v_gemm_rows_bf16(a, 60, a, 64, a, 64, 4, 64, 64, 0, None, 0, None), -2, g)  # ldx < K
    err(L.x2v_gemm_rows_bf16(a, 64, a, 64, a, 32, 4, 64, 64, 0, None, 0, None), -2, g)  # ldy < N ...
    assert L.x2v_gemm_rows_bf16(a, 64, a, 64, a, 32, 0, 32, 64, 3, None, 0, None) == 0  # ... but N = 32 GEGLU columns fit; no rows: nothing launched
    err(L.x2v_gemm_rows_bf16(odd, 64, a, 64, a, 64, 4, 64, 64, 0, None, 0, None), -2, g)  # alignment
    assert L.x2v_gemm_rows_bf16_tile_choice(0, 64, 0) == -1 and L.x2v_gemm_rows_bf16_tile_choice(4, 64, 7) == -1
    # the tile follows W's rows: the GEGLU weight of N output columns has 2N of them
    assert L.x2v_gemm_rows_bf16_tile_choice(203, 10240, 3) == L.x2v_gemm_rows_bf16_tile_choice(203, 20480, 0)
    assert lib.gemm_rows_bf16_tile_choice(203, 4096) == (64, 64) and lib.gemm_rows_bf16_tile_choice(77, 4096) == (64, 32)
    assert L.x2v_gemm_f16_tile_choice(203, 4096) == L.x2v_gemm_rows_bf16_tile_choice(203, 4096, 0)  # one rule for both element types

    # x2v_attn_bf16_d64_relbias(qkv, ld, bias, out, ldo, cu_seqlens, batch, heads, scale, stream)
    t = b"attn_bf16_d64_relbias"

    def cu(*v):
        return (ctypes.c_int * len(v))(*v)

    err(L.x2v_attn_bf16_d64_relbias(None, 768, a, a, 256, cu(0, 4), 1, 4, 1.0, None), -5, t)
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, None, 1, 4, 1.0, None), -5, t)
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, cu(*range(0, 40, 4)), 9, 4, 1.0, None), -1, t)  # batch 9
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, cu(0, 4), 0, 4, 1.0, None), -1, t)
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, cu(0, 513), 1, 4, 1.0, None), -1, t)  # length 513
    assert b"513" in L.x2v_last_error()
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, cu(0, 8, 8), 2, 4, 1.0, None), -1, t)  # not increasing
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, cu(0, 8, 5), 2, 4, 1.0, None), -1, t)
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, cu(-1, 8), 1, 4, 1.0, None), -1, t)
    err(L.x2v_attn_bf16_d64_relbias(a, 760, a, a, 256, cu(0, 8), 1, 4, 1.0, None), -2, t)  # ld below 3 * 4 * 64
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, odd, 256, cu(0, 8), 1, 4, 1.0, None), -2, t)
    err(L.x2v_attn_bf16_d64_relbias(a, 768, a, a, 256, cu(0, 8), 1, 4, float("nan"), None), -5, t)


def test_wrappers_refuse_on_the_host():
    """lib.gemm_rows_bf16 / attention_bf16_d64_relbias check dtypes and devices first: CPU tensors never reach a kernel (no fallback)."""
    from lightx2v_amd import lib

    x = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(lib.X2VError):
        lib.gemm_rows_bf16(x, x)
    with pytest.raises(lib.X2VError):
        lib.gemm_rows_bf16(x.half(), x.half())
    with pytest.raises(lib.X2VError):
        lib.attention_bf16_d64_relbias(torch.zeros(8, 768, dtype=torch.bfloat16), torch.zeros(4, 1023), [0, 8], 4)
