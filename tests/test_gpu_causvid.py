"""Wan CausVid on the GPU (lightx2v_amd/causvid.py) against the fixtures that tools/gen_golden_causvid.py recorded from the reference's
WanTransformerInferCausVid + WanStepDistillScheduler: wan-tiny and wan-tiny-i2v, 4 blocks of 45 tokens (kv_start 0, 45, 90, 135: three of the four
blocks start inside a 64-key V^T tile, two at odd offsets), 3 denoise steps each, the fixture's block latents and re-noise tensors injected.

Bounds are tests/test_gpu_model.py's for graphs of this depth: every noise_pred (one forward) within rel-L2 2e-2, every latents-after-step and
output_latents (the loop) within 3e-2.  Two further properties are bit comparisons: block 0 through the cache is the dense forward, and a block
re-run after later blocks wrote the cache gives the same bits."""
import os

import pytest
import torch

from tests.util import load_golden, record, rel_l2

pytestmark = pytest.mark.gpu

BLOCK_SHAPE, NUM_FRAMES, NUM_BLOCKS, STEP_LIST = (16, 3, 10, 6), 12, 4, [999, 756, 250]
TABLE = []


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    yield
    path = os.environ.get("X2V_CAUSVID_TABLE")  # where to write the measured figures (profiles/causvid_parity.txt is one run's)
    if path and TABLE:
        try:
            with open(path, "w") as f:
                f.write("# rel-L2 against the reference fixture (tests/golden/causvid_tiny*): bound 2e-2 for noise_pred, 3e-2 for latents and output_latents\n")
                f.write("\n".join(TABLE) + "\n")
        except OSError:
            pass


def build(task, ref_rounding, cls=None, **kw):
    from lightx2v_amd import causvid, scheduler, synth, wan

    name = "wan-tiny-i2v" if task == "i2v" else "wan-tiny"
    dims = synth.WAN_DIMS[name]
    wd = synth.synth_wan_i2v_weights(dims, seed=0) if task == "i2v" else synth.synth_wan_weights(dims, seed=0)
    extra = dict(task="i2v", in_dim=36, cross_attn_2_type="hip_flash") if task == "i2v" else {}
    cfg = wan.default_config(dims, target_shape=BLOCK_SHAPE, target_video_length=9, infer_steps=len(STEP_LIST), enable_cfg=False, sample_shift=8.0,
                             hip_ref_rounding=ref_rounding, denoising_step_list=list(STEP_LIST), num_frames=NUM_FRAMES, num_frame_per_block=BLOCK_SHAPE[1],
                             num_blocks=NUM_BLOCKS, frame_seq_length=15, **extra, **kw)
    model = (cls or causvid.WanCausVidModel)(cfg, {k: v.cuda() for k, v in wd.items()})
    sch = scheduler.WanStepDistillScheduler(cfg, device="cuda")
    model.set_scheduler(sch)
    return model, sch, cfg, wd


def inputs_of(g, task):
    inputs = {"text_encoder_output": {"context": [g["context"].cuda()]}}
    if task == "i2v":
        inputs["image_encoder_output"] = {"clip_encoder_out": g["clip_encoder_out"].cuda(), "vae_encode_out": g["vae_encode_out"].cuda()}
    return inputs


def fixture_noise(g, blocks=range(NUM_BLOCKS)):
    """noise_fn serving the fixture's re-noise tensors in the order step_post asks for them."""
    queue = [g[f"noise_b{b}_s{s}"] for b in blocks for s in range(len(STEP_LIST) - 1)]
    return lambda like: queue.pop(0).to(like.device)


@pytest.mark.parametrize("task", ["t2v", "i2v"])
def test_causvid_loop_against_the_reference_fixture(task):
    from lightx2v_amd import causvid
    from oracle.gen_golden import weights_checksum

    g = load_golden("causvid_tiny_i2v" if task == "i2v" else "causvid_tiny")
    model, sch, cfg, wd = build(task, True)
    assert torch.equal(weights_checksum(wd), g["weights_checksum"]), "synth weights drifted from the fixture's"
    sch.noise_fn = fixture_noise(g)
    rows = []

    def after_step(b, s):
        e_pred, e_lat = rel_l2(sch.noise_pred, g[f"noise_pred_b{b}_s{s}"]), rel_l2(sch.latents, g[f"latents_b{b}_s{s}"])
        rows.append((b, s, e_pred, e_lat, bool(torch.isfinite(sch.noise_pred).all())))

    out = causvid.run_causvid(model, sch, inputs_of(g, task), cfg, block_latents=lambda b: g[f"latents0_b{b}"], step_callback=after_step)
    assert torch.equal(sch.timesteps.cpu(), g["timesteps"])
    e_out = rel_l2(out, g["output_latents"])
    for b, s, e_pred, e_lat, _ in rows:
        print(f"{task} block {b} step {s}: noise_pred {e_pred:.3e} latents {e_lat:.3e}")
        TABLE.append(f"{task} block {b} (kv_start {45 * b}) step {s}: noise_pred {e_pred:.3e}  latents {e_lat:.3e}")
    print(f"{task} output_latents {e_out:.3e}")
    TABLE.append(f"{task} output_latents: {e_out:.3e}")
    record(f"causvid {task} 4 blocks x 3 steps (ref_rounding=True)", worst_noise_pred=max(r[2] for r in rows), worst_latents=max(r[3] for r in rows), output_latents=e_out)
    assert len(rows) == NUM_BLOCKS * len(STEP_LIST) and all(r[4] for r in rows)
    assert out.shape == (16, NUM_FRAMES, 10, 6) and out.dtype == torch.bfloat16
    assert max(r[2] for r in rows) <= 2e-2, [r[:3] for r in rows]
    assert max(r[3] for r in rows) <= 3e-2, [(r[0], r[1], r[3]) for r in rows]
    assert e_out <= 3e-2, e_out


def test_fractional_timesteps_keep_their_fraction_in_the_sinusoid():
    """The step-distill timesteps are sigma * 1000 in fp32 (999.87, 961.2, 727.3 at shift 8) and the reference embeds them unrounded (utils.py:161-172:
    float64 positions).  Truncating them to integers moved noise_pred by 9e-2 at step 999 — the term the loop test's first run was missing.  Against
    float64 torch at tests/test_gpu_ops.py's bar for the integer entry (one bf16 ulp + 1e-6 for the values near zero); integral floats give the
    integer entry's bits."""
    from lightx2v_amd import lib, scheduler, synth, wan
    from tests.util import assert_bf16_close

    cfg = wan.default_config(synth.WAN_DIMS["wan-tiny"], target_shape=BLOCK_SHAPE, sample_shift=8.0, denoising_step_list=list(STEP_LIST), infer_steps=3)
    sch = scheduler.WanStepDistillScheduler(cfg, device="cuda")
    sch.prepare(latents=torch.zeros(BLOCK_SHAPE))
    t = sch.timesteps
    assert t.dtype == torch.float32 and bool((t != t.round()).all())
    pos = t.cpu().to(torch.float64)
    sinusoid = torch.outer(pos, torch.pow(10000, -torch.arange(128).to(pos).div(128)))
    want = torch.cat([torch.cos(sinusoid), torch.sin(sinusoid)], dim=1).to(torch.bfloat16)
    assert_bf16_close(lib.sinusoid_embed(t, 256), want, ulps=1, atol=1e-6, bad_frac=5e-3, name="sinusoid of fractional timesteps")
    whole = torch.tensor([0, 1, 500, 999], device="cuda")
    assert torch.equal(lib.sinusoid_embed(whole.float(), 256), lib.sinusoid_embed(whole, 256))


def test_block0_through_the_cache_is_the_dense_forward():
    """kv_start = 0: the same kernels on the same operands as WanModel._forward (fp32-statistics mode, where the dense driver attends through the
    V^T kernel too) — projections, norm + RoPE at offset 0, V^T with a zero tail, attention with the PRESCALED flag alone."""
    from lightx2v_amd import wan

    g = load_golden("causvid_tiny")
    inputs = inputs_of(g, "t2v")
    model, sch, cfg, _ = build("t2v", False)
    dense, dsch, _, _ = build("t2v", False, cls=wan.WanModel)
    for m, s in ((model, sch), (dense, dsch)):
        s.prepare(latents=g["latents0_b0"])
        s.step_pre(1)
    model.init_kv_cache()
    model.infer(inputs, 0, 45)
    want = dense._forward(inputs, True)
    assert torch.isfinite(want).all() and torch.equal(sch.noise_pred, want)
    # and a block further on is NOT the dense forward of its own tokens: it sees block 0's keys
    sch.prepare(latents=g["latents0_b1"])
    sch.step_pre(1)
    model.infer(inputs, 45, 90)
    dsch.prepare(latents=g["latents0_b1"])
    dsch.step_pre(1)
    assert not torch.equal(sch.noise_pred, dense._forward(inputs, True))


@pytest.mark.parametrize("ref_rounding", [False, True])
def test_rerun_of_a_block_after_later_blocks_gives_the_same_bits(ref_rounding):
    """Blocks 0..3 run in order; then block 1's steps run again from the same latents and re-noise.  Its keys [0, 45) are what block 0 left and its own
    rows [45, 90) are rewritten by itself, so the noise_pred bits repeat exactly unless blocks 2 and 3 touched something outside their own ranges."""
    g = load_golden("causvid_tiny")
    inputs = inputs_of(g, "t2v")
    model, sch, cfg, _ = build("t2v", ref_rounding)
    model.init_kv_cache()

    def run_block(b):
        preds = []
        sch.prepare(latents=g[f"latents0_b{b}"])
        sch.noise_fn = fixture_noise(g, [b])
        for s in range(sch.infer_steps):
            sch.step_pre(s)
            model.infer(inputs, 45 * b, 45 * b + 45)
            preds.append(sch.noise_pred.clone())
            sch.step_post()
        return preds

    first = [run_block(b) for b in range(NUM_BLOCKS)]
    again = run_block(1)
    assert all(torch.isfinite(p).all() for p in again)
    assert all(torch.equal(a, b) for a, b in zip(again, first[1]))
    for layer in model.transformer_infer.kv_cache.layers:  # 180 keys in 3 tiles: the 12 key columns behind the last block are still the zero fill
        assert bool((layer["vt"][:, 2, :, 52:] == 0).all())


def test_refusals():
    from lightx2v_amd import wan

    g = load_golden("causvid_tiny")
    inputs = inputs_of(g, "t2v")
    model, sch, cfg, _ = build("t2v", False)
    sch.prepare(latents=g["latents0_b0"])
    sch.step_pre(0)
    tr = model.transformer_infer
    with pytest.raises(Exception, match="KV cache"):
        model.infer(inputs, 0, 45)
    model.init_kv_cache()
    for attr, value, word in (("parallel_attention", object(), "parallel attention"), ("_pair", (45, 64), "CFG pair"), ("radial", True, "hip_radial"), ("mx_attn", True, "hip_mxfp8")):
        old = getattr(tr, attr)
        setattr(tr, attr, value)
        try:
            with pytest.raises(NotImplementedError, match=word):
                model.infer(inputs, 0, 45)
        finally:
            setattr(tr, attr, old)
    model.config["enable_cfg"] = True
    with pytest.raises(NotImplementedError, match="enable_cfg"):
        model.infer(inputs, 0, 45)
    model.config["enable_cfg"] = False
    model.infer(inputs, 0, 45)  # and the plain call still runs
    assert torch.isfinite(sch.noise_pred).all()
    assert isinstance(model, wan.WanModel)
