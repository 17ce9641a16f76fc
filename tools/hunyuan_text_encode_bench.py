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


def median(v):
    return sorted(v)[len(v) // 2]


def hf_llama(sd, dims):
    """transformers' LlamaModel alone, as hf_models builds it, or None."""
    try:
        from transformers import LlamaConfig, LlamaModel
    except Exception:
        return None
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device("cuda"):
            ll = LlamaModel(LlamaConfig(vocab_size=dims["vocab"], hidden_size=dims["dim"], intermediate_size=dims["ffn"], num_hidden_layers=dims["layers"],
                                        num_attention_heads=dims["heads"], num_key_value_heads=dims["kv_heads"], head_dim=dims["head_dim"], rms_norm_eps=dims["eps"],
                                        rope_theta=dims["rope_theta"], max_position_embeddings=8192, hidden_act="silu", pad_token_id=None))
    finally:
        torch.set_default_dtype(old)
    ll.load_state_dict(sd, strict=True)
    return ll.eval().requires_grad_(False)


def gemm_mid_mode(a):
    """--gemm-mid.  Part one: the four Linears of a Llama layer at M = 351 and M = 130 through x2v_gemm_f16, x2v_gemm_mid_f16 and torch's fp16 matmul,
    interleaved A-B-A-B, each sample `--inner` launches between two device events, medians of `--rounds`; the whole block is repeated `--repeats` times
    and the spread of the repeated medians is reported.  Part two: the launch chain of infer_ids' forward (forward_packed on a filled workspace) and
    infer_ids itself with mid_gemm off and on, interleaved, repeated the same way, next to the plain-PyTorch and transformers towers."""
    from lightx2v_amd import lib, llama, synth
    from tests import llama_restatement as RL

    lib.init(0)
    res = {"device": torch.cuda.get_device_name(0), "box_calibration": {"kernel": "v_mfma_f32_16x16x32_bf16 (x2v_mfma_probe_bf16)", "mfma_probe_tflops_before": lib.mfma_probe(500)},
           "method": f"A-B-A-B in one process, device events, {a.inner} launches per sample, median of {a.rounds}, {a.repeats} repeats of every median"}
    D, A, Q, F = 4096, 4096, 6144, 14336
    g = torch.Generator().manual_seed(1)
    products = {"qkv": (Q, D, lib.EPI16_NONE), "o": (D, A, lib.EPI16_RESIDUAL), "gate_up_swiglu": (F, D, lib.EPI16_SWIGLU), "down": (D, F, lib.EPI16_RESIDUAL)}
    res["products"] = {}
    for name, (N, K, epi) in products.items():
        w = (torch.randn(2 * N if epi == lib.EPI16_SWIGLU else N, K, generator=g) / K**0.5).half().cuda()
        for M in (351, 130):
            x, r = torch.randn(M, K, generator=g).half().cuda(), torch.randn(M, N, generator=g).half().cuda()
            out, resid = torch.empty(M, N, dtype=torch.float16, device="cuda"), (r if epi == lib.EPI16_RESIDUAL else None)
            wt = w.t()
            arms = {"gemm_f16": lambda: lib.gemm_f16(x, w, None, epilogue=epi, resid=resid, out=out),
                    "gemm_mid_f16": lambda: lib.gemm_mid_f16(x, w, None, epilogue=epi, resid=resid, out=out),
                    "torch_matmul_fp16_no_epilogue": lambda: torch.matmul(x, wt)}
            for fn in arms.values():
                fn()
                fn()
            # results must not change: the two entries on the same operands (out of place), elements further apart than one fp16 ulp
            y_old, y_mid = (f(x, w, None, epilogue=epi, resid=resid).double() for f in (lib.gemm_f16, lib.gemm_mid_f16))
            apart = ((y_old - y_mid).abs() > 2.0**-10 * y_old.abs() + 2.0**-23).double().mean().item()
            meds = {k: [] for k in arms}
            for _ in range(a.repeats):
                ms = {k: [] for k in arms}
                for _ in range(a.rounds):
                    for k, fn in arms.items():
                        ms[k].append(timed_ms(lambda: [fn() for _ in range(a.inner)]) / a.inner)
                for k in arms:
                    meds[k].append(median(ms[k]))
            flop = 2.0 * M * w.shape[0] * K
            (tile, splits), mid, old = lib.gemm_mid_choice(M, w.shape[0], K), median(meds["gemm_mid_f16"]), median(meds["gemm_f16"])
            res["products"][f"{name}_M{M}"] = {"M": M, "W_rows": w.shape[0], "K": K, "tile": tile, "splits": splits, "ms_repeated_medians": meds,
                                               "ms": {k: median(v) for k, v in meds.items()}, "tflops": {k: flop / median(v) / 1e9 for k, v in meds.items()},
                                               "share_of_elements_over_1ulp_from_gemm_f16": apart, "gemm_f16_over_gemm_mid_f16": old / mid,
"gemm_mid_f16_over_torch": mid / median(meds["torch_matmul_fp16_no_epilogue"]),
                                               "spread_of_medians": {k: (max(v) - min(v)) / median(v) for k, v in meds.items()}}
        del w
    dims = dict(synth.LLAMA_DIMS["llama3-8b"], layers=a.layers)
    sd = synth.synth_llama_weights(dims, seed=0, device="cuda")
    models = {"mid_gemm_off": llama.TextEncoderHFLlamaModel((sd, dims), "cuda", mid_gemm=False), "mid_gemm_on": llama.TextEncoderHFLlamaModel((sd, dims), "cuda", mid_gemm=True)}
    g = torch.Generator().manual_seed(4)
    res["chain"] = {}
    hf = None if a.no_transformers else hf_llama(sd, dims)
    for n in (351, 130):
        ids, mask = torch.zeros(1, 351, dtype=torch.long), torch.zeros(1, 351, dtype=torch.long)
        ids[0, :n], mask[0, :n] = torch.randint(1, dims["vocab"], (n,), generator=g), 1
        dev = (ids.cuda(), mask.cuda())
        arms = {}
        for k, m in models.items():
            arms[f"infer_ids_{k}"] = lambda m=m: m.infer_ids(ids, mask)
            arms[f"chain_{k}"] = lambda m=m: m.forward_packed((n,))
        arms["torch_fp16_padded_351"] = lambda: RL.infer_ids(sd, dims, *dev, dtype=torch.float16, device="cuda", skip=2, crop_start=95)
        if hf is not None:
            arms["transformers_fp16_padded_351"] = lambda: hf(input_ids=dev[0], attention_mask=dev[1], output_hidden_states=True).hidden_states[-3][:, 95:]
        with torch.no_grad():
            for fn in arms.values():
                fn()
                fn()
            same = torch.equal(models["mid_gemm_on"].infer_ids(ids, mask)[0], models["mid_gemm_on"].infer_ids(ids, mask)[0])
            # results must not change.  At full depth the random-weight tower amplifies every rounding difference, so each path is held against the
            # fp32 restatement next to the plain-PyTorch fp16 path, and the switch is compared at 2 layers (the depth of the GPU tests) as well
            rel = lambda p, q: ((p.double() - q.double()).norm() / q.double().norm()).item()  # noqa: E731
            on, off = (models[k].infer_ids(ids, mask)[0][0, : n - 95] for k in ("mid_gemm_on", "mid_gemm_off"))
            truth, ref16 = (RL.infer_ids(sd, dims, *dev, dtype=t, device="cuda", skip=2, crop_start=95)[0][0, : n - 95] for t in (torch.float32, torch.float16))
            d2 = dict(dims, layers=4)
            on2, off2 = (llama.TextEncoderHFLlamaModel((sd, d2), "cuda", mid_gemm=s).infer_ids(ids, mask)[0][0, : n - 95] for s in (True, False))
            truth2 = RL.infer_ids(sd, d2, *dev, dtype=torch.float32, device="cuda", skip=2, crop_start=95)[0][0, : n - 95]
            parity = {"full_depth_vs_fp32": {"mid_gemm_on": rel(on, truth), "mid_gemm_off": rel(off, truth), "torch_fp16": rel(ref16, truth)},
                      "full_depth_on_vs_off": rel(on, off), "full_depth_off_vs_torch_fp16": rel(off, ref16),
                      "two_layers_vs_fp32": {"mid_gemm_on": rel(on2, truth2), "mid_gemm_off": rel(off2, truth2)}, "two_layers_on_vs_off": rel(on2, off2)}
            del truth, ref16, on2, off2, truth2
            meds = {k: [] for k in arms}
            for _ in range(a.repeats):
                ms = {k: [] for k in arms}
                for _ in range(a.rounds):
                    for k, fn in arms.items():
                        ms[k].append(timed_ms(fn))
                for k in arms:
                    meds[k].append(median(ms[k]))
        med = {k: median(v) for k, v in meds.items()}
        spread = {k: (max(v) - min(v)) / median(v) for k, v in meds.items()}
        gain = 1.0 - med["chain_mid_gemm_on"] / med["chain_mid_gemm_off"]
        res["chain"][f"llama_{n}"] = {"ms_repeated_medians": meds, "ms": med, "spread_of_medians": spread, "chain_gain_of_mid_gemm": gain,
                                      "chain_gain_exceeds_spread": gain > max(spread["chain_mid_gemm_on"], spread["chain_mid_gemm_off"]),
                                      "mid_gemm_on_run_to_run_bit_equal": same, "rel_l2": parity,
                                      "torch_fp16_over_hip": {k: med["torch_fp16_padded_351"] / med[f"infer_ids_{k}"] for k in models},
                                      **({"transformers_fp16_over_hip": {k: med["transformers_fp16_padded_351"] / med[f"infer_ids_{k}"] for k in models}} if hf is not None else {})}
    res["box_calibration"]["mfma_probe_tflops_after"] = lib.mfma_probe(500)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-transformers", action="store_true")
    ap.add_argument("--gemm-mid", action="store_true", help="time x2v_gemm_mid_f16 against x2v_gemm_f16: the four Llama products, then the chain with mid_gemm off and on")
    ap.add_argument("--inner", type=int, default=20, help="--gemm-mid: launches per timed sample of a single product")
    ap.add_argument("--repeats", type=int, default=3, help="--gemm-mid: how often every median is taken again (their spread gates the driver's default)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "gemm_mid_bench.json" if a.gemm_mid else "hunyuan_text_encode_bench.json")
    if a.gemm_mid:
        return gemm_mid_mode(a)
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
