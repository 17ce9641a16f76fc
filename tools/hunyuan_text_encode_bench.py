#!/usr/bin/env python
"""Times HunyuanVideo's two text towers on the HIP kernels (lightx2v_amd/llama.py, lightx2v_amd/clip_text.py: released dims, weights drawn on the GPU) —
the Llama tower on a prompt of 351 and one of 130 valid tokens, the CLIP-L text tower with the end token at position 76 and at 20 (77 and 21 tokens run) —
warmed up, HIP events, medians — and in the same process, interleaved A-B-A-B, the same towers in fp16 through plain PyTorch on the same GPU run as the
reference runs them: padded to max_length (351 / 77), ids and mask on the GPU (tests/llama_restatement.py, tests/clip_text_restatement.py).  If transformers
imports, LlamaModel / CLIPTextModel themselves (fp16, the library's default attention) are timed the same way on the same weights.  Reports ms, Linear
weight bytes / time, the ratio to the streaming floor weight_bytes() / 6.29 TB/s (DESIGN §4's measured HBM rate) and the launch count; writes one JSON
object to --out and prints it.
    python tools/hunyuan_text_encode_bench.py [--rounds 5] [--layers 32] [--out profiles/hunyuan_text_encode_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.29


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def hf_models(sd_l, dims_l, sd_c, dims_c):
    """transformers' own models in fp16 on the GPU with the same weights, or None."""
    try:
        from transformers import CLIPTextConfig, CLIPTextModel, LlamaConfig, LlamaModel
    except Exception:
        return None
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device("cuda"):
            ll = LlamaModel(LlamaConfig(vocab_size=dims_l["vocab"], hidden_size=dims_l["dim"], intermediate_size=dims_l["ffn"], num_hidden_layers=dims_l["layers"],
                                        num_attention_heads=dims_l["heads"], num_key_value_heads=dims_l["kv_heads"], head_dim=dims_l["head_dim"], rms_norm_eps=dims_l["eps"],
                                        rope_theta=dims_l["rope_theta"], max_position_embeddings=8192, hidden_act="silu", pad_token_id=None))
            cl = CLIPTextModel(CLIPTextConfig(vocab_size=dims_c["vocab"], hidden_size=dims_c["dim"], intermediate_size=dims_c["ffn"], num_hidden_layers=dims_c["layers"],
                                              num_attention_heads=dims_c["heads"], max_position_embeddings=dims_c["positions"], hidden_act="quick_gelu",
                                              layer_norm_eps=dims_c["eps"], eos_token_id=dims_c["eos_token_id"], bos_token_id=1, pad_token_id=1))
    finally:
        torch.set_default_dtype(old)
    ll.load_state_dict(sd_l, strict=True)
    probe = "text_model.embeddings.token_embedding.weight"
    cl.load_state_dict(sd_c if probe in cl.state_dict() else {k[len("text_model."):]: v for k, v in sd_c.items()}, strict=True)
    return ll.eval().requires_grad_(False), cl.eval().requires_grad_(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-transformers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hunyuan_text_encode_bench.json"))
    a = ap.parse_args()
    from lightx2v_amd import clip_text, lib, llama, synth
    from tests import clip_text_restatement as RC
    from tests import llama_restatement as RL

    lib.init(0)
    dims_l = dict(synth.LLAMA_DIMS["llama3-8b"], layers=a.layers)
    dims_c = synth.CLIP_TEXT_DIMS["clip-l"]
    sd_l, sd_c = synth.synth_llama_weights(dims_l, seed=0, device="cuda"), synth.synth_clip_text_weights(dims_c, seed=0, device="cuda")
    ml, mc = llama.TextEncoderHFLlamaModel((sd_l, dims_l), "cuda"), clip_text.TextEncoderHFClipModel((sd_c, dims_c), "cuda")
    g = torch.Generator().manual_seed(4)
    prompts_l, prompts_c = {}, {}
    for n in (351, 130):
        ids, mask = torch.zeros(1, ml.max_length, dtype=torch.long), torch.zeros(1, ml.max_length, dtype=torch.long)
        ids[0, :n], mask[0, :n] = torch.randint(1, dims_l["vocab"], (n,), generator=g), 1
        prompts_l[n] = (ids, mask)
    end = dims_c["vocab"] - 1
    for n in (77, 21):
        ids, mask = torch.full((1, mc.max_length), end, dtype=torch.long), torch.zeros(1, mc.max_length, dtype=torch.long)
        ids[0, : n - 1], mask[0, :n] = torch.randint(1, end, (n - 1,), generator=g), 1
        prompts_c[n] = (ids, mask)
    dev_l = {n: tuple(t.cuda() for t in p) for n, p in prompts_l.items()}  # the baselines' inputs as the reference holds them at its forward: on the GPU
    dev_c = {n: tuple(t.cuda() for t in p) for n, p in prompts_c.items()}
    skip, crop = ml.hidden_state_skip_layer, ml.crop_start

    cases = {}
    for n in prompts_l:
        cases[f"llama_hip_{n}"] = lambda n=n: ml.infer_ids(*prompts_l[n])
        cases[f"llama_torch_fp16_{n}_padded_351"] = lambda n=n: RL.infer_ids(sd_l, dims_l, *dev_l[n], dtype=torch.float16, device="cuda", skip=skip, crop_start=crop)
    for n in prompts_c:
        cases[f"clip_hip_{n}"] = lambda n=n: mc.infer_ids(*prompts_c[n])
        cases[f"clip_torch_fp16_{n}_padded_77"] = lambda n=n: RC.infer_ids(sd_c, dims_c, *dev_c[n], dtype=torch.float16, device="cuda")
    hf = None if a.no_transformers else hf_models(sd_l, dims_l, sd_c, dims_c)
    if hf is not None:
        for n in prompts_l:
            cases[f"llama_transformers_fp16_{n}_padded_351"] = lambda n=n: hf[0](input_ids=dev_l[n][0], attention_mask=dev_l[n][1], output_hidden_states=True).hidden_states[-(skip + 1)][:, crop:]
        for n in prompts_c:
            cases[f"clip_transformers_fp16_{n}_padded_77"] = lambda n=n: hf[1](input_ids=dev_c[n][0], attention_mask=dev_c[n][1], output_hidden_states=False)["pooler_output"]
    with torch.no_grad():
        for fn in cases.values():  # warm-up: allocations, lazy module load, launch plans
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in cases}
        for _ in range(a.rounds):  # A-B-A-B: the paths alternate inside one process
            for k, fn in cases.items():
                ms[k].append(timed_ms(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    # the launch chains alone (no host-side id checks, gather or output copies) on a filled workspace
    chain = {}
    for n in prompts_l:
        ml.infer_ids(*prompts_l[n])
        chain[f"llama_{n}"] = sorted(timed_ms(lambda: ml.forward_packed((n,))) for _ in range(5))[2]
    for n in prompts_c:
        mc.infer_ids(*prompts_c[n])
        chain[f"clip_{n}"] = sorted(timed_ms(lambda: mc.forward_packed((n,))) for _ in range(5))[2]
    wb = {"llama": ml.weight_bytes(), "clip": mc.weight_bytes()}
    floor = {k: v / (HBM_TBS * 1e12) * 1e3 for k, v in wb.items()}
    res = {"workload": f"HunyuanVideo text towers, fp16: Llama-3-8B dims, {ml.num_layers} of {a.layers} layers, 351 and 130 valid tokens; CLIP-L text, 12 layers, 77 and 21 tokens",
           "weight_bytes": wb, "weight_stream_floor_ms_at_6.29TBs": floor, "launches_per_forward": {"llama": ml.launches(), "clip": mc.launches()},
           "ms_median": med, "ms_all": ms, "hip_chain_only_ms": chain,
           "hip_chain_over_weight_floor": {k: v / floor[k.split("_")[0]] for k, v in chain.items()},
           "hip_chain_weight_gbs": {k: wb[k.split("_")[0]] / v / 1e6 for k, v in chain.items()},
           "torch_fp16_over_hip": {**{f"llama_{n}": med[f"llama_torch_fp16_{n}_padded_351"] / med[f"llama_hip_{n}"] for n in prompts_l},
                                   **{f"clip_{n}": med[f"clip_torch_fp16_{n}_padded_77"] / med[f"clip_hip_{n}"] for n in prompts_c}},
           "tflops_per_s_chain": {**{f"llama_{n}": llama.encoder_flops(ml, (n,)) / chain[f"llama_{n}"] / 1e9 for n in prompts_l},
                                  **{f"clip_{n}": clip_text.encoder_flops(mc, (n,)) / chain[f"clip_{n}"] / 1e9 for n in prompts_c}}}
    if hf is not None:
        res["transformers_fp16_over_hip"] = {**{f"llama_{n}": med[f"llama_transformers_fp16_{n}_padded_351"] / med[f"llama_hip_{n}"] for n in prompts_l},
                                             **{f"clip_{n}": med[f"clip_transformers_fp16_{n}_padded_77"] / med[f"clip_hip_{n}"] for n in prompts_c}}
        import transformers

        res["transformers_version"] = transformers.__version__
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
