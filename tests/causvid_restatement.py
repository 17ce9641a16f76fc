"""The reference's causal block loop (wan_causvid_runner.py:75-130 for num_fragments == 1, causvid_model.py:55-58, infer/causvid/transformer_infer.py,
step_distill/scheduler.py) restated on the functions of oracle/wan_oracle.py, which is imported and not edited.

The oracle's `wan_block` already has the two hooks the causal block needs, through its `sp = (rank, world, attn_fn)` argument:
  * RoPE: compute_freqs_dist(s, c, grid, freqs, rank, world) takes rows [rank * s, (rank + 1) * s) of the table of `grid`.  With s = the block's
    tokens, rank = the block index j, world = j + 1 and grid = (kv_end // (h w), h, w) these are the rows of frames [kv_start // (h w), kv_end // (h w))
    and nothing is padded — compute_freqs_causvid(..., start_frame = kv_start // (h w)) of transformer_infer.py:104;
  * attention: attn_fn(q, k, v) stores k and v into the layer's cache rows [kv_start, kv_end) and attends q over rows [0, kv_end) (:112-127).
Everything else of the causal block is the dense block's arithmetic written out of place (x = x + y * gate for x.add_(y * gate), and so on): the
same bf16 operations in the same order.  tests/test_causvid_host.py pins this file to tests/golden/causvid_tiny*."""
import torch

from oracle import wan_oracle as O

BLOCK_SHAPE, NUM_FRAMES, NUM_BLOCKS = (16, 3, 10, 6), 12, 4


def weights_of(task):
    from lightx2v_amd import synth

    name = "wan-tiny-i2v" if task == "i2v" else "wan-tiny"
    dims = synth.WAN_DIMS[name]
    return dims, (synth.synth_wan_i2v_weights(dims, seed=0) if task == "i2v" else synth.synth_wan_weights(dims, seed=0))


def causal_forward(wd, dims, caches, latents_bf16, t, context_list, kv_start, kv_end, image=None):
    """causvid_model.py:55-58: pre-infer (i2v: with the block's frames of vae_encode_out, pre_infer.py:47-52), the causal blocks, post-infer."""
    if image is not None:
        ve = image["vae_encode_out"]
        fsl = (ve.size(2) // 2) * (ve.size(3) // 2)
        if kv_end - kv_start >= fsl:
            image = dict(image, vae_encode_out=ve[:, kv_start // fsl : kv_end // fsl])
    embed, grid, x, embed0, s, context = O.wan_pre_infer(wd, dims, latents_bf16, t, context_list, image=image)
    assert s == kv_end - kv_start
    H, d = dims["num_heads"], dims["dim"] // dims["num_heads"]
    freqs = O.rope_freqs_table(d)
    per_frame = grid[1] * grid[2]
    j, rem = divmod(kv_start, s)
    assert rem == 0 and kv_start % per_frame == 0 and kv_end % per_frame == 0
    causal_grid = (kv_end // per_frame, grid[1], grid[2])

    def attend_into(cache):
        def fn(q, k, v):
            cache["k"][kv_start:kv_end] = k
            cache["v"][kv_start:kv_end] = v
            return O.sdpa(q, cache["k"][:kv_end], cache["v"][:kv_end])

        return fn

    for i in range(dims["num_layers"]):
        x = O.wan_block(wd, i, dims, causal_grid, x, embed0, freqs, context, sp=(j, j + 1, attend_into(caches[i])))
    return O.wan_post_infer(wd, x, embed, grid)


def run(g, task):
    """The fixture's run restated: its block latents and re-noise tensors in, {noise_pred_b*_s*, latents_b*_s*, output_latents} out."""
    dims, wd = weights_of(task)
    H, d = dims["num_heads"], dims["dim"] // dims["num_heads"]
    fsl = (BLOCK_SHAPE[2] // 2) * (BLOCK_SHAPE[3] // 2)
    per_block = BLOCK_SHAPE[1] * fsl
    caches = [{"k": torch.zeros(NUM_FRAMES * fsl, H, d, dtype=torch.bfloat16), "v": torch.zeros(NUM_FRAMES * fsl, H, d, dtype=torch.bfloat16)} for _ in range(dims["num_layers"])]
    image = {"clip_encoder_out": g["clip_encoder_out"], "vae_encode_out": g["vae_encode_out"]} if task == "i2v" else None
    timesteps, sigmas = g["timesteps"], g["sigmas"]
    steps = timesteps.numel()
    out = {}
    output_latents = torch.zeros((16, NUM_FRAMES, *BLOCK_SHAPE[2:]), dtype=torch.bfloat16)
    with torch.no_grad():
        for b in range(NUM_BLOCKS):
            kv_start, kv_end = b * per_block, (b + 1) * per_block
            latents = g[f"latents0_b{b}"].clone()  # step_distill/scheduler.py:42-43: reset() redraws
            for s in range(steps):
                latents = latents.to(torch.bfloat16)  # step_pre
                pred = causal_forward(wd, dims, caches, latents, torch.stack([timesteps[s]]), [g["context"]], kv_start, kv_end, image)
                # step_distill/scheduler.py:49-56
                x0 = latents.to(torch.float32) - sigmas[s].item() * pred.to(torch.float32)
                if s < steps - 1:
                    noise, nxt = g[f"noise_b{b}_s{s}"], sigmas[s + 1].item()
                    x0 = ((1 - nxt) * x0 + nxt * noise).type_as(noise)
                latents = x0.to(latents.dtype)
                out[f"noise_pred_b{b}_s{s}"], out[f"latents_b{b}_s{s}"] = pred, latents.clone()
            output_latents[:, b * BLOCK_SHAPE[1] : (b + 1) * BLOCK_SHAPE[1]] = latents
    out["output_latents"] = output_latents
    return out
