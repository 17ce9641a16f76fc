"""Wan CausVid without a GPU: the causal block loop restated on the functions of oracle/wan_oracle.py (tests/causvid_restatement.py) against the
fixture recorded from the reference (tests/golden/causvid_tiny*), and the host logic of lightx2v_amd.causvid.run_causvid with a stub model — offsets,
latents redrawn per block, output_latents assembly, refusals."""
import pytest
import torch

from tests import causvid_restatement as CR
from tests.util import load_golden, rel_l2

BLOCK_SHAPE = (16, 3, 10, 6)


def config(**kw):
    from lightx2v_amd import synth, wan

    cfg = wan.default_config(synth.WAN_DIMS["wan-tiny"], target_shape=BLOCK_SHAPE, enable_cfg=False, sample_shift=8.0, infer_steps=3, denoising_step_list=[999, 756, 250],
                             num_frames=12, num_frame_per_block=3, num_blocks=4, frame_seq_length=15)
    cfg.update(kw)
    return cfg


class StubModel:
    """What run_causvid asks of a model: init_kv_cache(capacity) and infer(inputs, kv_start, kv_end) leaving scheduler.noise_pred."""

    def __init__(self, scheduler):
        self.scheduler, self.calls, self.capacity, self.seen_latents = scheduler, [], None, []

    def init_kv_cache(self, capacity=None):
        self.capacity = capacity
        self.calls.append("init")

    def infer(self, inputs, kv_start, kv_end):
        sch = self.scheduler
        self.calls.append((kv_start, kv_end, sch.step_index))
        self.seen_latents.append(sch.latents.clone())
        assert sch.latents.dtype == torch.bfloat16  # step_pre ran
        sch.noise_pred = torch.full(BLOCK_SHAPE, 0.25 * (1 + kv_start // 45))


def test_run_causvid_offsets_latents_and_assembly():
    from lightx2v_amd import causvid, scheduler

    cfg = config()
    assert causvid.causvid_plan(cfg) == (15, 45, [(0, 45), (45, 90), (90, 135), (135, 180)], 180)
    sch = scheduler.WanStepDistillScheduler(cfg, device="cpu", noise_fn=lambda x: torch.zeros_like(x, dtype=torch.float32))
    model = StubModel(sch)
    lats = [torch.full(BLOCK_SHAPE, float(b + 1)) for b in range(4)]
    seen = []
    out = causvid.run_causvid(model, sch, {}, cfg, block_latents=lats, step_callback=lambda b, s: seen.append((b, s)))
    assert model.calls[0] == "init" and model.capacity == 180
    assert model.calls[1:] == [(45 * b, 45 * b + 45, s) for b in range(4) for s in range(3)]
    assert seen == [(b, s) for b in range(4) for s in range(3)]
    # latents redrawn per block: the first step of block b sees lats[b], not what block b - 1 left
    for b in range(4):
        assert torch.equal(model.seen_latents[3 * b].float(), lats[b])
    # assembly: block b's final latents in frames [3 b, 3 b + 3); with zero re-noise the loop is x <- (1 - s_next) (x - s v), then x - s v
    assert out.shape == (16, 12, 10, 6) and out.dtype == torch.bfloat16
    sig = sch.sigmas.tolist()
    for b in range(4):
        x, v = torch.tensor(float(b + 1)), 0.25 * (b + 1)
        for s in range(3):
            x = x.to(torch.bfloat16).float() - sig[s] * v
            if s < 2:
                x = (1 - sig[s + 1]) * x
            x = x.to(torch.bfloat16).float()
        blk = out[:, 3 * b : 3 * b + 3].float()
        assert bool((blk == blk.flatten()[0]).all()) and abs(blk.flatten()[0].item() - x.item()) <= 2 ** -7 * abs(x.item())
    # default latents: one seeded generator, a fresh draw per block
    model2 = StubModel(sch)
    causvid.run_causvid(model2, sch, {}, cfg)
    firsts = [model2.seen_latents[3 * b] for b in range(4)]
    assert all(not torch.equal(firsts[0], f) for f in firsts[1:])
    model3 = StubModel(sch)
    causvid.run_causvid(model3, sch, {}, cfg)
    assert all(torch.equal(a, b) for a, b in zip(model2.seen_latents, model3.seen_latents))  # seeded: reproducible


def test_fewer_blocks_than_frames_leave_the_rest_zero():
    from lightx2v_amd import causvid, scheduler

    cfg = config(num_blocks=2)
    sch = scheduler.WanStepDistillScheduler(cfg, device="cpu")
    out = causvid.run_causvid(StubModel(sch), sch, {}, cfg)
    assert bool((out[:, 6:] == 0).all()) and bool((out[:, :6] != 0).any())


def test_refusals_of_the_runner_and_the_plan():
    from lightx2v_amd import causvid, scheduler

    with pytest.raises(NotImplementedError, match="num_fragments"):
        causvid.causvid_plan(config(num_fragments=3))
    with pytest.raises(ValueError, match="num_frame_per_block"):
        causvid.causvid_plan(config(num_frame_per_block=4))
    with pytest.raises(ValueError, match="frame_seq_length"):
        causvid.causvid_plan(config(frame_seq_length=1560))
    with pytest.raises(ValueError, match="num_blocks"):
        causvid.causvid_plan(config(num_blocks=5))
    cfg = config()
    sch = scheduler.WanStepDistillScheduler(cfg, device="cpu")
    with pytest.raises(ValueError, match="latents"):
        causvid.run_causvid(StubModel(sch), sch, {}, cfg, block_latents=[torch.zeros(16, 2, 10, 6)] * 4)
    with pytest.raises(NotImplementedError, match="num_fragments"):
        causvid.run_causvid(StubModel(sch), sch, {}, config(num_fragments=2))


def test_driver_refusals_need_no_gpu():
    """The combinations the causal driver does not build are refused before any kernel runs."""
    from lightx2v_amd import causvid

    tr = causvid.WanTransformerInferCausVid(config())

    class W:  # the one thing the check reads from the weights: block 0's k projection
        class _B:
            class _P:
                class self_attn_k:
                    @staticmethod
                    def apply(x):
                        return x

            compute_phases = [None, _P]

        blocks = [_B]

    for attr, value, word in (("parallel_attention", object(), "parallel attention"), ("_pair", (45, 64), "CFG pair"), ("radial", True, "hip_radial"), ("mx_attn", True, "hip_mxfp8")):
        old = getattr(tr, attr)
        setattr(tr, attr, value)
        with pytest.raises(NotImplementedError, match=word):
            tr.infer(W, None, None, torch.zeros(45, 256), None, None, None, None, 0, 45)
        setattr(tr, attr, old)
    with pytest.raises(NotImplementedError, match="out="):
        tr.infer(W, None, None, torch.zeros(45, 256), None, None, None, None, 0, 45)


# ---- the restated loop against the reference fixture ----
@pytest.mark.parametrize("task", ["t2v", "i2v"])
def test_restated_causal_loop_reproduces_the_reference_fixture(task):
    g = load_golden("causvid_tiny_i2v" if task == "i2v" else "causvid_tiny")
    got = CR.run(g, task)
    worst = 0.0
    for k in sorted(got):
        if not torch.equal(got[k], g[k]):
            worst = max(worst, rel_l2(got[k], g[k]))
    assert set(got) == {k for k in g if k.startswith(("noise_pred_b", "latents_b", "output_latents"))}
    assert worst == 0.0, f"restatement differs from the reference fixture: worst rel-L2 {worst:.3e}"
