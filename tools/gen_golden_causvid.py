"""Generates tests/golden/causvid_tiny.*.safetensors and causvid_tiny_i2v.*.safetensors from the unmodified reference's autoregressive Wan:
WanTransformerInferCausVid (models/networks/wan/infer/causvid/transformer_infer.py) with the reference's WanPreInfer / WanPostInfer and its
WanStepDistillScheduler (schedulers/wan/step_distill/scheduler.py), on CPU in bf16, `torch_sdpa` attention, `Default` linear layers.

Workload: synth `wan-tiny` / `wan-tiny-i2v` weights (seed 0; only their checksum is stored), latent block shape (16, 3, 10, 6) — frame_seq_length 15,
45 tokens per block — num_frames 12, num_blocks 4, denoising_step_list [999, 756, 250], sample_shift 8, no CFG.  kv_start is 0, 45, 90, 135: the
first-tile remainders of the 64-key V^T tile are 0, 45, 26, 7 — every block but the first starts mid-tile, two offsets are odd, and kv_end = 135
spans three tiles.

Stored, per fixture: `latents0_b<j>` the latents each block starts from (the scheduler's reset() draw); `noise_b<j>_s<i>` every re-noise tensor of
step_post, recorded by a wrapper around torch.randn_like that returns the reference's own draw unchanged; `noise_pred_b<j>_s<i>` and
`latents_b<j>_s<i>` after every (block, step); `output_latents`; timesteps and sigmas; the contexts (and for i2v clip_encoder_out / vae_encode_out);
`weights_checksum`.

What is NOT the reference's code here:
  * the block loop: wan_causvid_runner.py:75-130 `run()` for num_fragments == 1 and causvid_model.py:55-58 `infer()` are restated as the few lines of
    `run_reference` (their classes load checkpoints, a VAE and text encoders in their constructors); every object they call is the reference's;
  * `scheduler.device = cpu`, and the kv cache allocated with device="cpu" (the runner passes "cuda");
  * the recording wrapper around torch.randn_like (no arithmetic), after torch.manual_seed(SEED) — the reference draws the re-noise from the
    unseeded global RNG;
  * what oracle.ref_import.patch_and_import() patches for every reference import.
`python tools/gen_golden_causvid.py` (needs the reference checkout that oracle/ref_import.py finds)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lightx2v_amd import synth  # noqa: E402
from oracle import ref_import  # noqa: E402
from oracle.gen_golden import save_golden, weights_checksum  # noqa: E402

SEED = 1234
BLOCK_SHAPE = (16, 3, 10, 6)
NUM_FRAMES, NUM_BLOCKS = 12, 4
STEP_LIST = [999, 756, 250]


def causvid_overrides(task):
    ts = BLOCK_SHAPE
    fsl = (ts[2] // 2) * (ts[3] // 2)
    o = dict(target_shape=ts, enable_cfg=False, sample_shift=8.0, infer_steps=len(STEP_LIST), denoising_step_list=list(STEP_LIST), num_frames=NUM_FRAMES,
             num_frame_per_block=ts[1], num_blocks=NUM_BLOCKS, frame_seq_length=fsl, num_fragments=1, task=task, seed=42)
    if task == "i2v":
        o.update(in_dim=36, lat_h=ts[2], lat_w=ts[3])
    return o


def run_reference(task):
    ref_import.patch_and_import()
    from lightx2v.models.networks.wan.infer.causvid.transformer_infer import WanTransformerInferCausVid
    from lightx2v.models.schedulers.wan.step_distill.scheduler import WanStepDistillScheduler

    name = "wan-tiny-i2v" if task == "i2v" else "wan-tiny"
    dims = synth.WAN_DIMS[name]
    wd = synth.synth_wan_i2v_weights(dims, seed=0) if task == "i2v" else synth.synth_wan_weights(dims, seed=0)
    cfg = ref_import.make_config(dims, **causvid_overrides(task))
    R = ref_import.build_reference_wan(cfg, wd)
    tr = R["tr"] = WanTransformerInferCausVid(cfg)
    _, ctx, _ = synth.synth_inputs(dims, BLOCK_SHAPE)
    inputs = {"text_encoder_output": {"context": ctx}}
    out = dict(weights_checksum=weights_checksum(wd), context=ctx[0])
    image = None
    if task == "i2v":
        image = synth.synth_i2v_inputs(dims, (16, NUM_FRAMES, BLOCK_SHAPE[2], BLOCK_SHAPE[3]))
        inputs["image_encoder_output"] = image
        out.update(clip_encoder_out=image["clip_encoder_out"], vae_encode_out=image["vae_encode_out"])
    sch = WanStepDistillScheduler(cfg)
    sch.device = torch.device("cpu")
    sch.prepare(image)
    for m in ("pre", "post", "tr"):
        R[m].set_scheduler(sch)
    out.update(timesteps=sch.timesteps.clone(), sigmas=sch.sigmas.clone())

    drawn = []
    real_randn_like = torch.randn_like

    def recording_randn_like(*a, **k):
        t = real_randn_like(*a, **k)
        drawn.append(t.clone())
        return t

    torch.manual_seed(SEED)
    torch.randn_like = recording_randn_like
    try:
        with torch.no_grad():
            # wan_causvid_runner.py:75-130, num_fragments == 1
            tr._init_kv_cache(dtype=torch.bfloat16, device="cpu")
            tr._init_crossattn_cache(dtype=torch.bfloat16, device="cpu")
            nfpb, fsl = cfg.num_frame_per_block, cfg.frame_seq_length
            output_latents = torch.zeros((cfg.target_shape[0], cfg.num_frames, *cfg.target_shape[2:]), dtype=torch.bfloat16)
            kv_start, kv_end = 0, nfpb * fsl
            for block_idx in range(cfg.num_blocks):
                sch.reset()
                out[f"latents0_b{block_idx}"] = sch.latents.clone()
                for step_index in range(sch.infer_steps):
                    sch.step_pre(step_index=step_index)
                    # causvid_model.py:55-58
                    embed, grid_sizes, pre_out = R["pre"].infer(R["pre_w"], inputs, positive=True, kv_start=kv_start, kv_end=kv_end)
                    x = tr.infer(R["tr_w"], grid_sizes, embed, *pre_out, kv_start, kv_end)
                    sch.noise_pred = R["post"].infer(R["post_w"], x, embed, grid_sizes)[0]
                    n_before = len(drawn)
                    sch.step_post()
                    if len(drawn) > n_before:
                        assert len(drawn) == n_before + 1
                        out[f"noise_b{block_idx}_s{step_index}"] = drawn[-1]
                    out[f"noise_pred_b{block_idx}_s{step_index}"] = sch.noise_pred.clone()
                    out[f"latents_b{block_idx}_s{step_index}"] = sch.latents.clone()
                kv_start += nfpb * fsl
                kv_end += nfpb * fsl
                output_latents[:, block_idx * nfpb : (block_idx + 1) * nfpb] = sch.latents
            out["output_latents"] = output_latents
    finally:
        torch.randn_like = real_randn_like
    return out


def main():
    for task, name in (("t2v", "causvid_tiny"), ("i2v", "causvid_tiny_i2v")):
        out = run_reference(task)
        save_golden(out, name)
        nbytes = sum(v.numel() * v.element_size() for v in out.values())
        print(f"{name}.*.safetensors: {len(out)} tensors, {nbytes} bytes;", {k: (tuple(v.shape), str(v.dtype)) for k, v in out.items() if k.startswith(("output", "latents0_b0", "noise_b0_s0"))})


if __name__ == "__main__":
    main()
