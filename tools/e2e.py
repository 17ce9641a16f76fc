#!/usr/bin/env python
"""End-to-end wall clock of the hot path on one GPU: the full denoise loop (all infer_steps, CFG) followed by the VAE decode of the
final latents — the quantity BASELINE.json's north star asks for next to the per-step number ("end-to-end wall-clock and frames/sec").
Synthetic weights and inputs of the named shape (the text encoder's output is an input here, as in bench.py, unless --t5 is given).  One JSON line.
    python tools/e2e.py [--workload wan14b_720px81f] [--steps 50] [--fp8|--int8|--mxfp8|--mxfp6|--mxfp4] [--distill] [--teacache T]
    python tools/e2e.py --i2v --image PATH | --encode   (image → CLIP tower + VAE encode → loop → decode; --encode: a seeded synthetic 720p image;
                                                         --clip-ckpt PATH: the CLIP checkpoint instead of seeded synthetic tower weights)
    python tools/e2e.py --causvid --workload wan1.3b_480px81f   (the autoregressive Wan: 7 blocks of 3 latent frames, 9 steps each, over a KV cache; then the decode)
    python tools/e2e.py --t5   (context / context_null from seeded token ids through the HIP umT5-XXL encoder, seeded weights, timed as t5_encode_s)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/e2e.py --gpus N ...
        (N GPUs of one node: Ulysses sequence parallel denoise loop over RCCL + the halo-split `decode_dist` VAE decode)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import lib, scheduler, synth, vae, wan  # noqa: E402


CAUSVID_STEP_LIST = [999, 934, 862, 756, 603, 410, 250, 140, 74]  # configs/causvid/wan_t2v_causvid.json of the reference


def causvid_main(a):
    """--causvid: the reference's `wan2.1_causvid` run (configs/causvid/wan_t2v_causvid.json: 21 latent frames in 7 blocks of 3, 9 distilled steps per
    block, no CFG, shift 8) on the workload's latent grid, then the VAE decode of the assembled latents.  One JSON line; `block_s` is the wall clock of
    each autoregressive block (9 steps), fenced by a device synchronise."""
    from lightx2v_amd import causvid

    if a.gpus != 1:
        raise SystemExit("--causvid: single GPU (the causal driver has no parallel attention, as the reference)")
    torch.cuda.set_device(0)
    lib.init(0)
    wl = synth.WORKLOADS[a.workload]
    dims = synth.WAN_DIMS[wl["model"]]
    if dims.get("task") == "i2v":
        raise SystemExit("--causvid: a t2v workload (the i2v path is covered by the parity tests)")
    _, T, h, w = wl["target_shape"]
    nfpb = 3
    blocks = a.causvid_blocks or T // nfpb
    steps = CAUSVID_STEP_LIST[: a.steps] if a.steps else CAUSVID_STEP_LIST
    ts = (16, nfpb, h, w)
    fsl = (h // 2) * (w // 2)
    extra = {}
    if a.fp8:
        extra["mm_config"] = {"mm_type": "W-fp8-channel-sym-A-fp8-channel-sym-dynamic-Hip", "weight_auto_quant": True}
    if a.int8:
        extra["mm_config"] = {"mm_type": "W-int8-channel-sym-A-int8-channel-sym-dynamic-Hip", "weight_auto_quant": True}
    _, _, wd, _, inputs = synth.workload_setup(a.workload, seed=0, device="cuda")
    cfg = wan.default_config(dims, target_shape=ts, target_video_length=wl["frames"], infer_steps=len(steps), enable_cfg=False, sample_shift=8.0, denoising_step_list=steps,
                             num_frames=T, num_frame_per_block=nfpb, num_blocks=blocks, frame_seq_length=fsl, num_fragments=1, **extra)
    model = causvid.WanCausVidModel(cfg, wd)
    del wd
    sch = scheduler.WanStepDistillScheduler(cfg, device="cuda")
    model.set_scheduler(sch)
    decoder = vae.WanVAE(synth.synth_wan_vae_weights(dim=96, seed=0), dim=96, conv16=(True if a.vae16 else False if a.vae32 else "split"), use_tiling=a.tiling_vae)
    # warm-up outside the clock: one block (allocator pools, lazy tables, the cross-attention K / V) and a short decode
    warm = dict(cfg, num_blocks=1)
    causvid.run_causvid(model, sch, inputs, warm)
    decoder.decode(torch.zeros(16, 2, h, w, device="cuda"))
    torch.cuda.synchronize()
    marks = []

    def after_step(b, s):
        if s == len(steps) - 1:
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

    t0 = time.perf_counter()
    latents = causvid.run_causvid(model, sch, inputs, cfg, step_callback=after_step)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    video = decoder.decode(latents[:, : blocks * nfpb].float())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert torch.isfinite(latents.float()).all() and torch.isfinite(video).all()
    block_s = [b - a_ for a_, b in zip([t0] + marks[:-1], marks)]  # block 0 includes the cache allocation
    frames = 1 + 4 * (blocks * nfpb - 1)
    print(json.dumps({"workload": a.workload, "mode": "causvid", "latent_frames": blocks * nfpb, "output_latents_shape": list(latents.shape), "blocks": blocks, "frames_per_block": nfpb,
                      "steps_per_block": len(steps), "tokens_per_block": nfpb * fsl, "kv_capacity": T * fsl, "cfg": False,
                      "gemm_dtype": "int8" if a.int8 else "fp8" if a.fp8 else "bf16", "denoise_s": t1 - t0, "block_s": block_s, "ms_per_step_by_block": [x * 1e3 / len(steps) for x in block_s],
                      "vae_decode_s": t2 - t1, "total_s": t2 - t0, "frames": frames, "video_shape": list(video.shape), "fps_with_vae": frames / (t2 - t0),
                      "hbm_gb_peak": torch.cuda.max_memory_allocated() / 1e9, "data": "synthetic weights / latents / text embeddings"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--causvid", action="store_true", help="the autoregressive Wan (wan2.1_causvid): blocks of 3 latent frames, 9 distilled steps each, over a per-layer KV cache; use a 21-latent-frame t2v workload such as wan1.3b_480px81f; single GPU")
    ap.add_argument("--causvid-blocks", type=int, default=0, help="--causvid: number of blocks (default: all the workload's latent frames / 3)")
    ap.add_argument("--workload", default="wan14b_720px81f")
    ap.add_argument("--steps", type=int, default=0, help="0 = the workload's own schedule length (50; 40 for the i2v benchmark workloads)")
    ap.add_argument("--i2v", action="store_true", help="--workload wan14b_i2v_720px81f: the reference's published benchmark (I2V-14B, 40 steps, CFG 5, shift 5; configs/bench/lightx2v_2.json)")
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--int8", action="store_true", help="w8a8 int8 linear layers (the reference's int8 presets), weights quantised at load")
    ap.add_argument("--mxfp8", action="store_true")
    ap.add_argument("--mxfp6", action="store_true", help="MXFP6 (e3m2) weights x MXFP8 activations, weights quantised at load")
    ap.add_argument("--mxfp4", action="store_true", help="MXFP4 (e2m1) weights x MXFP4 activations, weights quantised at load (every linear K a multiple of 256)")
    ap.add_argument("--distill", action="store_true", help="4-step distilled schedule, no CFG (BASELINE config #4)")
    ap.add_argument("--vae16", action="store_true", help="fastest VAE decode: convolution operands rounded to fp16")
    ap.add_argument("--vae32", action="store_true", help="VAE convolutions on the fp32 matrix instruction (default: hi/lo fp16 split, fp32-grade)")
    ap.add_argument("--tiling-vae", action="store_true", help='the reference configs\' "use_tiling_vae": WanVAE(use_tiling=True) — tiled decode (and encode with --image / --encode)')
    ap.add_argument("--tiny-vae", action="store_true", help='the reference configs\' "tiny_vae": decode with WanVAE_tiny (TAEHV, lightx2v_amd/vae_tiny.py) instead of WanVAE; single GPU')
    ap.add_argument("--tiny-vae-ckpt", default=None, help="--tiny-vae: the released taew2_1.pth (default: seeded synthetic weights)")
    ap.add_argument("--teacache", type=float, default=0.0, help="TeaCache threshold (0 = off); uses the released 14B 720p coefficients")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--ring", action="store_true", help='with --gpus N: parallel_attn_type="ring" (ring attention: no num_heads %% N constraint) instead of "ulysses"')
    ap.add_argument("--radial", type=int, default=0, metavar="ROUNDS", help='time ROUNDS denoise steps with "self_attn_1_type": "hip_radial" next to ROUNDS dense steps (A-B-A-B, same model, same process) and print that instead of a full run; single GPU')
    ap.add_argument("--mx-attn", type=int, nargs="?", const=5, default=0, metavar="ROUNDS", help='time ROUNDS (default 5) denoise steps with "self_attn_1_type": "hip_mxfp8" (block-scaled fp8 self-attention) next to ROUNDS dense steps (A-B-A-B, same model, same process) and print that instead of a full run; single GPU')
    ap.add_argument("--image", default=None, help="i2v: build clip_encoder_out / vae_encode_out from this image (PIL) with the HIP CLIP tower / VAE encoder, timed as clip_encode_s / vae_encode_s")
    ap.add_argument("--clip-ckpt", default=None, help="i2v with --image / --encode: CLIP checkpoint (.pth / .safetensors) for the HIP image tower (default: seeded synthetic weights)")
    ap.add_argument("--encode", action="store_true", help="i2v: as --image, on a seeded synthetic image of the workload's size")
    ap.add_argument("--t5", action="store_true", help="build context / context_null from seeded token ids (77- and 126-token prompts) with the HIP umT5-XXL encoder (seeded weights), timed as t5_encode_s")
    a = ap.parse_args()
    if a.causvid:
        return causvid_main(a)
    from lightx2v_amd import launch

    world, rank, local_rank = launch.ranks(__file__, a.gpus)  # bare `--gpus N`: re-runs itself as N ranks under torch.distributed.run
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch.distributed as dist

        if launch.one_gpu_test():  # plumbing mode (lightx2v_amd/launch.py): all ranks on one GPU over gloo with host-staged collectives, timings meaningless
            dist.init_process_group("gloo")
            launch.host_staged_collectives(dist)
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    lib.init(local_rank)
    if a.i2v:
        a.workload = "wan14b_i2v_720px81f"
    wl = synth.WORKLOADS[a.workload]
    dims = synth.WAN_DIMS[wl["model"]]
    steps = 4 if a.distill else (a.steps or wl.get("infer_steps", 50))
    extra = {}
    if a.fp8:
        extra["mm_config"] = {"mm_type": "W-fp8-channel-sym-A-fp8-channel-sym-dynamic-Hip", "weight_auto_quant": True}
    if a.int8:
        extra["mm_config"] = {"mm_type": "W-int8-channel-sym-A-int8-channel-sym-dynamic-Hip", "weight_auto_quant": True}
    if a.mxfp8:
        extra["mm_config"] = {"mm_type": "W-mxfp8-A-mxfp8-dynamic-Hip", "weight_auto_quant": True}
    if a.mxfp6:
        extra["mm_config"] = {"mm_type": "W-mxfp6-A-mxfp8-dynamic-Hip", "weight_auto_quant": True}
    if a.mxfp4:
        extra["mm_config"] = {"mm_type": "W-mxfp4-A-mxfp4-dynamic-Hip", "weight_auto_quant": True}
    if a.distill:
        extra.update(enable_cfg=False, denoising_step_list=[1000, 750, 500, 250], sample_shift=5.0)
    if a.teacache > 0:
        # configs/caching/teacache/wan_t2v_tea_720p.json of the reference: coefficients for Wan2.1-T2V-14B 720p
        extra.update(feature_caching="Tea", teacache_thresh=a.teacache, use_ret_steps=False,
                     coefficients=[[8.10705460e03, 2.13393892e03, -3.72934672e02, 1.66203073e01, -4.17769401e-02],
                                   [-114.36346466, 65.26524496, -18.82220707, 4.91518089, -0.23412683]])
    if world > 1 and a.ring:
        extra["parallel_attn_type"] = "ring"
    elif world > 1:
        if dims["num_heads"] % world:
            raise SystemExit(f"Ulysses needs num_heads % N == 0 ({dims['num_heads']} heads, N={world}); --ring has no such constraint")
        extra["parallel_attn_type"] = "ulysses"
    _, overrides, wd, lat, inputs = synth.workload_setup(a.workload, seed=0, device="cuda")  # i2v: the i2v checkpoint + seeded CLIP / VAE-encode stand-ins
    extra = {**overrides, **extra}
    cfg = wan.default_config(dims, target_shape=wl["target_shape"], target_video_length=wl["frames"], infer_steps=steps, **extra)
    model = wan.WanModel(cfg, wd)
    del wd
    sch = (scheduler.WanStepDistillScheduler if a.distill else scheduler.WanScheduler)(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    encode = (a.image is not None or a.encode) and dims.get("task") == "i2v"
    vae_sd = synth.synth_wan_vae_weights(dim=96, seed=0)
    if encode:  # one VAE state dict with both halves, as the released Wan2.1_VAE.pth
        vae_sd = {**vae_sd, **synth.synth_wan_vae_encoder_weights(dim=96, seed=0)}
    decoder = vae.WanVAE(vae_sd, dim=96, conv16=(True if a.vae16 else False if a.vae32 else "split"), parallel=world > 1,
                         use_tiling=a.tiling_vae)
    encoder_vae = decoder  # the i2v conditioning is encoded by the full VAE in either case
    if a.tiny_vae:  # WanRunner.load_vae_decoder (wan_runner.py:136-150): the tiny decoder replaces the full one on the decode side only
        from lightx2v_amd import vae_tiny

        if world > 1:
            raise SystemExit("--tiny-vae: the tiny decoder has no multi-GPU form")
        decoder = vae_tiny.WanVAE_tiny(a.tiny_vae_ckpt or synth.synth_taehv_weights(seed=0))
    if encode:
        from lightx2v_amd import clip, vae_enc

        clip_model = clip.CLIPModel(torch.float16, "cuda", a.clip_ckpt or synth.synth_clip_weights(synth.CLIP_DIMS["clip-vit-h-14"], seed=0, device="cuda"), False, None, None)
        _, _, th, tw = wl["target_shape"]
        if a.image is not None:  # TF.to_tensor(img).sub_(0.5).div_(0.5) of run_vae_encoder (wan_runner.py:205)
            import numpy as np
            from PIL import Image

            img = torch.from_numpy(np.asarray(Image.open(a.image).convert("RGB"), dtype=np.float32) / 255.0).permute(2, 0, 1).sub_(0.5).div_(0.5)
        else:
            img = torch.rand(3, 8 * th, 8 * tw, generator=torch.Generator().manual_seed(0)) * 2 - 1
        enc_args = dict(target_height=8 * th, target_width=8 * tw, target_video_length=wl["frames"], vae_stride=cfg["vae_stride"], patch_size=cfg["patch_size"])
        if vae_enc.i2v_latent_hw(img.shape[1], img.shape[2], 8 * th, 8 * tw, cfg["vae_stride"], cfg["patch_size"]) != (th, tw):
            raise SystemExit(f"--image: a {img.shape[2]}x{img.shape[1]} image gives another latent grid than the workload's {tw}x{th} (use the workload's aspect ratio)")
        vae_enc.run_vae_encoder(encoder_vae, img, **enc_args)  # warm-up: allocates the encoder's buffers
        clip.run_image_encoder(clip_model, img.cuda())
    if a.t5:
        from lightx2v_amd import t5

        if dims.get("text_dim", 4096) != synth.T5_DIMS["umt5-xxl"]["dim"]:
            raise SystemExit(f"--t5: the workload's text_dim {dims.get('text_dim')} is not umT5-XXL's {synth.T5_DIMS['umt5-xxl']['dim']}")
        t5_model = t5.T5EncoderModel(dims.get("text_len", 512), torch.bfloat16, "cuda", synth.synth_t5_weights(synth.T5_DIMS["umt5-xxl"], seed=0, device="cuda"))
        gt = torch.Generator().manual_seed(7)
        t5_ids = [torch.randint(1, synth.T5_DIMS["umt5-xxl"]["vocab"], (1, n), generator=gt) for n in (77, 126)]  # prompt, negative prompt
        t5_args = (t5_ids[0], torch.ones_like(t5_ids[0]), t5_ids[1], torch.ones_like(t5_ids[1]))
        t5.run_text_encoder(t5_model, *t5_args)  # warm-up: allocates the encoder's workspace
    # warm-up outside the clock: one step on a scratch scheduler state (allocator pools, lazy tables) and a short decode
    sch.step_pre(0)
    model.infer(inputs)
    decoder.decode(torch.zeros(16, 2, wl["target_shape"][2], wl["target_shape"][3], device="cuda"))
    sch.reset() if hasattr(sch, "reset") else None
    sch.prepare(latents=lat)
    if a.teacache > 0:
        model.transformer_infer.cnt = 0

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    if a.radial:
        # One model, two self-attention forms: the driver's switch is flipped between steps (with it on, the CFG forwards run one after the other —
        # the pair pass is dense-only — so each column is the step a user of that configuration gets).  Every step is step 0 of the schedule.
        if world > 1:
            raise SystemExit("--radial: single GPU (radial attention under Ulysses is not built)")
        tr, ms = model.transformer_infer, {False: [], True: []}
        for on in (False, True):  # warm both forms (the mask and its plan are built here)
            tr.radial = on
            sch.step_pre(0)
            model.infer(inputs)
        fence()
        for _ in range(a.radial):
            for on in (False, True):
                tr.radial = on
                sch.step_pre(0)
                fence()
                t0 = time.perf_counter()
                model.infer(inputs)
                fence()
                ms[on].append((time.perf_counter() - t0) * 1e3)
        med = {on: sorted(v)[len(v) // 2] for on, v in ms.items()}
        plan = next(iter(tr.mask_map._hip_plans.values()))
        tr.radial = False
        dense_form = "single forward" if not cfg["enable_cfg"] else "CFG pair pass" if model._pair_ok(inputs) else "two forwards (the size rule's form for this shape)"
        nb = (plan.seq_len + 127) // 128
        print(json.dumps({"workload": a.workload, "rounds": a.radial, "cfg": bool(cfg["enable_cfg"]), "dense_step_ms": med[False], "dense_step_ms_all": ms[False],
                          "radial_step_ms": med[True], "radial_step_ms_all": ms[True], "radial_over_dense": med[True] / med[False], "mask_density": plan.kept_blocks / float(nb * nb),
                          "dense_step_form": dense_form, "radial_step_form": "two forwards, one after the other" if cfg["enable_cfg"] else "single forward",
                          "data": "synthetic weights / latents / text embeddings"}))
        return
    if a.mx_attn:
        # As --radial: one model, the driver's switch flipped between steps.  With hip_mxfp8 on, the CFG forwards never take the pair pass (it is dense-only);
        # they run on two streams or one after the other by the size rule, so each column is the step a user of that configuration gets.  Every step is
        # step 0 of the schedule.
        if world > 1:
            raise SystemExit("--mx-attn: single GPU (block-scaled fp8 attention under Ulysses is not built)")
        tr, ms = model.transformer_infer, {False: [], True: []}
        for on in (False, True):
            tr.mx_attn = on
            sch.step_pre(0)
            model.infer(inputs)
        fence()
        for _ in range(a.mx_attn):
            for on in (False, True):
                tr.mx_attn = on
                sch.step_pre(0)
                fence()
                t0 = time.perf_counter()
                model.infer(inputs)
                fence()
                ms[on].append((time.perf_counter() - t0) * 1e3)
        med = {on: sorted(v)[len(v) // 2] for on, v in ms.items()}
        tr.mx_attn = False
        two = "two forwards on two compute streams" if wan.cfg_form_by_size(sch.seq_len, tr.num_heads) == "streams" else "two forwards, one after the other"
        dense_form = "single forward" if not cfg["enable_cfg"] else "CFG pair pass" if model._pair_ok(inputs) else two
        print(json.dumps({"workload": a.workload, "rounds": a.mx_attn, "cfg": bool(cfg["enable_cfg"]), "dense_step_ms": med[False], "dense_step_ms_all": ms[False],
                          "mx_step_ms": med[True], "mx_step_ms_all": ms[True], "mx_over_dense": med[True] / med[False], "box_mfma_tflops": lib.mfma_probe(500),
                          "dense_step_form": dense_form, "mx_step_form": two if cfg["enable_cfg"] else "single forward",
                          "data": "synthetic weights / latents / text embeddings"}))
        return
    fence()
    tt = time.perf_counter()
    if a.t5:  # WanRunner.run_text_encoder (wan_runner.py:178-191): both prompts in one packed pass
        inputs["text_encoder_output"] = dict(inputs["text_encoder_output"], **t5.run_text_encoder(t5_model, *t5_args))
        fence()
    te = time.perf_counter()
    tc = te
    if encode:  # WanRunner.run_image_encoder → run_vae_encoder (wan_runner.py:191-248)
        inputs["image_encoder_output"]["clip_encoder_out"] = clip.run_image_encoder(clip_model, img.cuda())
        fence()
        tc = time.perf_counter()
        inputs["image_encoder_output"]["vae_encode_out"] = vae_enc.run_vae_encoder(encoder_vae, img, **enc_args)[0]
        fence()
    t0 = time.perf_counter()
    scheduler.run_denoise_loop(model, sch, inputs)
    fence()
    t1 = time.perf_counter()
    video = decoder.decode(sch.latents.float())
    fence()
    t2 = time.perf_counter()
    assert torch.isfinite(video).all() and torch.isfinite(sch.latents).all()
    frames = wl["frames"]
    rec = {"workload": a.workload, "task": dims.get("task", "t2v"), "guide_scale": cfg["sample_guide_scale"], "sample_shift": cfg["sample_shift"], "n_gpus": world, "parallelism": f"{'ring' if a.ring else 'ulysses'}-sp{world} + decode_dist" if world > 1 else "single", "steps": steps, "cfg": bool(cfg["enable_cfg"]), "gemm_dtype": "mxfp4" if a.mxfp4 else "mxfp6xmxfp8" if a.mxfp6 else "mxfp8" if a.mxfp8 else "int8" if a.int8 else "fp8" if a.fp8 else "bf16",
           "teacache_thresh": a.teacache, "vae_conv_operands": "bf16 (tiny VAE / TAEHV)" if a.tiny_vae else "fp16" if a.vae16 else "fp32" if a.vae32 else "fp16 hi/lo split (fp32-grade)", "tiny_vae": bool(a.tiny_vae), "vae_tiling": bool(a.tiling_vae and world == 1), "denoise_s": t1 - t0, "ms_per_step": (t1 - t0) * 1e3 / steps, "vae_decode_s": t2 - t1, "total_s": t2 - t0,
           "frames": frames, "video_shape": list(video.shape), "fps_denoise_only": frames / (t1 - t0), "fps_with_vae": frames / (t2 - t0),
           "hbm_gb_peak": torch.cuda.max_memory_allocated() / 1e9, "data": "synthetic weights / latents / text embeddings"}
    if encode:  # both conditioning tensors were built from the image here
        rec.update(clip_encode_s=tc - te, vae_encode_s=t0 - tc, total_with_encode_s=t2 - te,
                   conditioning=(f"image {os.path.basename(a.image)}" if a.image else "seeded synthetic image") + ": clip_encoder_out from the HIP CLIP tower (" +
                   (f"checkpoint {os.path.basename(a.clip_ckpt)}" if a.clip_ckpt else "seeded synthetic weights") + "), vae_encode_out from the HIP VAE encoder")
    if a.t5:
        rec.update(t5_encode_s=te - tt, text_conditioning="context / context_null from seeded token ids (77 / 126 tokens) through the HIP umT5-XXL encoder, seeded weights")
    if a.teacache > 0:
        rec_c, rec_u = list(getattr(sch, "caching_records", [])), list(getattr(sch, "caching_records_2", []))
        rec["teacache_forwards_computed"] = int(sum(bool(v) for v in rec_c + rec_u))
        rec["teacache_forwards_total"] = len(rec_c) + len(rec_u)
    if rank == 0:
        print(json.dumps(rec))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
