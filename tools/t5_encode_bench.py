#!/usr/bin/env python
"""Times the umT5-XXL text encoder on the HIP kernels (lightx2v_amd/t5.py: released dims, weights drawn on the GPU) for a 77-token and a 126-token prompt in
one packed pass (what run_text_encoder does for prompt + negative prompt) and for the 77-token prompt alone — warmed up, HIP events — and in the same
process, interleaved A-B-A-B, the same encoder in bf16 through plain PyTorch on the same GPU run as the reference runs it: each prompt padded to 512 tokens,
one forward per prompt (tests/t5_restatement.py; its ids and mask are on the GPU and its delta -> bucket map is built before the clock starts, so the timed
baseline holds no host work beyond PyTorch's own launches).  Reports ms, Linear weight bytes / time against the streaming rate `tools/x2v_check hbm` measures in the same
session (run first, as a child process; --hbm-gbs overrides) and against DESIGN §4's 6.29 TB/s.  One JSON line.
    python tools/t5_encode_bench.py [--rounds 3] [--layers 24]"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.29


def session_hbm_gbs():
    """The best streaming rate among the BENCH lines of `tools/x2v_check hbm` (a child process, before this one touches the GPU); None if the tool is not built."""
    tool = os.path.join(ROOT, "tools", "x2v_check")
    if not os.path.exists(tool):
        return None
    out = subprocess.run([tool, "hbm"], capture_output=True, text=True, timeout=300).stdout
    rates = [float(v) for v in re.findall(r"([0-9.]+) GB/s", out)]
    return max(rates) if rates else None


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--hbm-gbs", type=float, default=0.0)
    a = ap.parse_args()
    hbm = a.hbm_gbs or session_hbm_gbs()
    from lightx2v_amd import lib, synth, t5
    from tests import t5_restatement as R

    lib.init(0)
    dims = dict(synth.T5_DIMS["umt5-xxl"], layers=a.layers)
    sd = synth.synth_t5_weights(dims, seed=0, device="cuda")
    m = t5.T5EncoderModel(512, torch.bfloat16, "cuda", sd)
    g = torch.Generator().manual_seed(4)
    prompts = []
    for n in (77, 126):
        ids = torch.randint(1, dims["vocab"], (1, n), generator=g)
        prompts.append((ids, torch.ones_like(ids)))
    # the baseline's inputs as the reference holds them at its forward: ids and mask on the GPU (model.py:586-587); the delta -> bucket map, which the
    # reference evaluates on the GPU inside each block, is built once here and left out of the clock (in the baseline's favour)
    padded = [tuple(t.cuda() for t in R.pad_to(i, k, 512)) for i, k in prompts]
    lens = [n for n in (77, 126)]
    buckets = R.bucket_map(512, dims["buckets"], "cuda")

    def torch_forward(j):
        return R.encoder(sd, *padded[j], dtype=torch.bfloat16, device="cuda", rel_buckets=buckets)[0, : lens[j]]

    def hip_pair():
        return t5.run_text_encoder(m, *prompts[0], *prompts[1])

    def hip_single():
        return m.infer_ids(*prompts[0])

    def torch_pair():
        with torch.no_grad():
            return [torch_forward(0), torch_forward(1)]

    def torch_single():
        with torch.no_grad():
            return torch_forward(0)

    cases = {"hip_pair_77_126": hip_pair, "torch_bf16_pair_padded_512": torch_pair, "hip_single_77": hip_single, "torch_bf16_single_padded_512": torch_single}
    for fn in cases.values():  # warm-up: allocations, lazy module load, kernel attributes
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.rounds):  # A-B-A-B: the two paths alternate inside one process
        for k, fn in cases.items():
            ms[k].append(timed_ms(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    # the blocks alone (no host-side id checks, gather or output copies): the launch chain on a filled workspace
    hip_pair()  # leaves the M = 203 workspace filled
    chain = sorted(timed_ms(lambda: m.forward_packed((77, 126))) for _ in range(5))[2]
    wb = m.weight_bytes()
    floor = wb / (HBM_TBS * 1e12) * 1e3
    res = {"workload": f"umT5-XXL encoder, {a.layers} blocks, bf16: prompts of 77 + 126 tokens in one packed pass, and 77 alone", "weight_bytes": wb,
           "weight_stream_floor_ms_at_6.29TBs": floor, "session_hbm_gbs": hbm, "launches_per_forward": 7 * a.layers + 1, "ms_median": med, "ms_all": ms,
           "hip_chain_only_pair_ms": chain, "torch_over_hip_pair": med["torch_bf16_pair_padded_512"] / med["hip_pair_77_126"],
           "torch_over_hip_single": med["torch_bf16_single_padded_512"] / med["hip_single_77"], "hip_chain_over_weight_floor": chain / floor,
           "hip_pair_weight_gbs": wb / chain / 1e6, "hip_pair_fraction_of_session_hbm": (wb / chain / 1e6 / hbm) if hbm else None,
           "tflops_per_s_pair": t5.encoder_flops(m, (77, 126)) / chain / 1e9}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
