#!/usr/bin/env python
"""Write tests/golden/radial_masks.npz: the block masks of the UNMODIFIED reference's radial attention (attentions/common/radial_attn.py, MaskMap),
run on the CPU from the reference checkout that oracle/ref_import.py locates.  Authoring-time only: the tests read the file, never the reference.

Per case: `mask_<k>` = np.packbits of the bool [n, n] mask, row-major, and `meta` = JSON list of {tokens_per_frame, frames, model_type, decay_factor,
n, seconds} in the same order.  The query handed to queryLogMask has the padded length ceil(S / 128) * 128, as radial_attn() pads it.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    (200, 9, "wan", 1),
    (260, 11, "wan", 1),
    (96, 24, "wan", 1),
    (70, 4, "wan", 1),
    (384, 8, "wan", 1),
    (150, 16, "wan", 1),
    (1560, 13, "wan", 1),
    (1560, 21, "wan", 1),
    (3600, 21, "wan", 1),
    (200, 9, "hunyuan", 1),
    (200, 9, "wan", 0.5),
]


def load_reference_module():
    from oracle import ref_import

    path = os.path.join(ref_import.REFERENCE_ROOT, "lightx2v", "attentions", "common", "radial_attn.py")
    spec = importlib.util.spec_from_file_location("reference_radial_attn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_mask(mod, tpf, frames, model_type, decay_factor):
    S = tpf * frames
    query = torch.empty(((S + 127) // 128 * 128, 1, 1))
    with contextlib.redirect_stdout(io.StringIO()):  # the reference prints the sparsity
        return mod.MaskMap(S, frames).queryLogMask(query, "radial", block_size=128, decay_factor=decay_factor, model_type=model_type)


def main():
    mod = load_reference_module()
    arrays, meta = {}, []
    for k, (tpf, frames, model_type, decay) in enumerate(CASES):
        t0 = time.time()
        m = reference_mask(mod, tpf, frames, model_type, decay).numpy()
        dt = time.time() - t0
        arrays[f"mask_{k}"] = np.packbits(m.reshape(-1))
        meta.append(dict(tokens_per_frame=tpf, frames=frames, model_type=model_type, decay_factor=decay, n=int(m.shape[0]), seconds=round(dt, 2)))
        print(f"{tpf} x {frames} {model_type} decay {decay}: {m.shape[0]} blocks per side, density {m.mean():.3f}, {dt:.1f} s", flush=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, "tests", "golden", "radial_masks.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
