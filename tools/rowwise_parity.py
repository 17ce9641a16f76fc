#!/usr/bin/env python3
"""One sha256 per case over every public entry of csrc/norm.hip and csrc/quant8.hip on seeded inputs, for comparing two builds of the
library bit for bit (a refactor against its parent commit):

    python tools/rowwise_parity.py path/to/parent/libx2v_hip.so > parent.txt
    python tools/rowwise_parity.py lightx2v_amd/libx2v_hip.so   > new.txt        (a fresh process per library)
    diff parent.txt new.txt

Row lengths 8 (one wave per row), 512, 520 (four waves, a partial chunk), 1536, 3072, 5120, 8192 and 13824 (CH = 8 with dead chunks); 37 and 4 rows;
the per-row (1) and streaming (2) variants wherever the streaming one is accepted; every LayerNorm operand set; both round modes of every RMS
entry; RMSNorm + RoPE with and without weights, the last rows past the rotation grid, q_out_scale 1 and 0.1275, the blocked entry at 2 and 40
heads; headnorm + RoPE with l_rope 0, L / 2 and L, the blocked entry with fewer heads per block than heads; both quantisers plain and K-blocked;
the fused LayerNorm + quantise entries.  Every input has an all-zero row (int8 inv = 0, the e4m3 floor scale) and a row with a 1e4 outlier."""
import hashlib
import os
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
os.environ["X2V_LIB_PATH"] = os.path.abspath(sys.argv[1])  # read by lightx2v_amd.lib at import
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from lightx2v_amd import lib  # noqa: E402

BF16 = torch.bfloat16
GEN = torch.Generator().manual_seed(20261)
DS = (8, 512, 520, 1536, 3072, 5120, 8192, 13824)
MS = (37, 4)
ROUNDS = (lib.ROUND_FP32, lib.ROUND_REF)


def rand(*shape, scale=1.0):
    return (torch.randn(*shape, generator=GEN) * scale).to(BF16).cuda()


def rows(M, D):
    """[M, D] with row 0 all zero and a 1e4 outlier in row 1"""
    x = torch.randn(M, D, generator=GEN)
    x[0] = 0
    x[1, (3 * D) // 7] = 1e4
    return x.to(BF16).cuda()


def emit(name, *tensors):
    h = hashlib.sha256()
    torch.cuda.synchronize()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    print(f"{name:88s} {h.hexdigest()}")


def run_rmsnorm():
    for D in DS:
        w = rand(D)
        for M in MS:
            x = rows(M, D)
            for rm in ROUNDS:
                emit(f"rmsnorm D={D} M={M} round={rm}", lib.rmsnorm(x, w, round_mode=rm))


def run_layernorm():
    for D in DS:
        w, b, sc, sh = rand(D), rand(D, scale=0.1), rand(D, scale=0.1), rand(D, scale=0.1)
        sets = {"plain": {}, "w": dict(weight=w), "b": dict(bias=b), "affine": dict(weight=w, bias=b), "modulate": dict(scale=sc, shift=sh),
                "affine+modulate": dict(weight=w, bias=b, scale=sc, shift=sh)}
        for M in MS:
            x = rows(M, D)
            for what, kw in sets.items():
                for variant in (0, 1, 2):
                    if variant == 2 and not 512 < D <= 8192:
                        continue
                    emit(f"layernorm {what} D={D} M={M} variant={variant}", lib.layernorm(x, variant=variant, **kw))
                if D > 512:
                    emit(f"layernorm_quant_fp8 {what} D={D} M={M}", *lib.layernorm_quant_fp8(x, **kw))
                    emit(f"layernorm_quant_int8 {what} D={D} M={M}", *lib.layernorm_quant_int8(x, **kw))


def rope_table():
    a = torch.randn(1024, 64, generator=GEN, dtype=torch.float64) * 3.0
    return torch.stack([a.cos(), a.sin()], dim=-1).float().contiguous().cuda()


def run_rmsnorm_rope():
    cs = rope_table()
    grid = (2, 3, 5)  # 30 tokens
    for H in (4, 12, 24, 40, 64, 108):
        D = H * 128
        wq, wk = rand(D), rand(D)
        for M in MS:
            s0 = 30 - M + min(M // 2, 7)  # the last rows fall past the grid
            q0, k0 = rows(M, D), rows(M, D)
            for rm in ROUNDS:
                for with_w in (True, False):
                    for qs in (1.0, 0.1275):
                        for variant in (0, 1, 2):
                            if variant == 2 and D > 8192:
                                continue
                            q, k = q0.clone(), k0.clone()
                            lib.rmsnorm_rope_(q, k, wq if with_w else None, wk if with_w else None, cs, grid, H, s0=s0, round_mode=rm, q_out_scale=qs, variant=variant)
                            emit(f"rmsnorm_rope H={H} M={M} round={rm} w={int(with_w)} qs={qs} variant={variant}", q, k)
    for H in (2, 40):
        D = H * 128
        wq, wk = rand(D), rand(D)
        for M in MS:
            q0, k0 = rows(M, D), rows(M, D)
            for rm in ROUNDS:
                for with_w in (True, False):
                    qo, ko = torch.zeros(2, M, D // 2, dtype=BF16, device="cuda"), torch.zeros(2, M, D // 2, dtype=BF16, device="cuda")
                    lib.rmsnorm_rope_blocked(q0, k0, wq if with_w else None, wk if with_w else None, cs, grid, H, qo, ko, s0=30 - M + min(M // 2, 7), round_mode=rm, q_out_scale=0.1275)
                    emit(f"rmsnorm_rope_blocked H={H} M={M} round={rm} w={int(with_w)}", qo, ko)


def run_headnorm_rope():
    wq, wk = rand(128), rand(128)
    for L in MS:
        cos, sin = rand(L, 128), rand(L, 128)
        for H, blocks in ((3, 1), (4, 2)):
            D = H * 128
            q0, k0 = rows(L, D), rows(L, D)
            for l_rope in (0, L // 2, L):
                for rm in ROUNDS:
                    for with_w in (True, False):
                        for qs in (1.0, 0.1275):
                            args = (wq if with_w else None, wk if with_w else None, cos, sin, H, l_rope)
                            name = f"H={H} L={L} l_rope={l_rope} round={rm} w={int(with_w)} qs={qs}"
                            q, k = q0.clone(), k0.clone()
                            lib.headnorm_rope_(q, k, *args, round_mode=rm, q_out_scale=qs)
                            emit(f"headnorm_rope {name}", q, k)
                            if blocks > 1:  # the same values, head-blocked [N, L, (H / N) * 128]
                                q = q0.view(L, blocks, D // blocks).transpose(0, 1).contiguous()
                                k = k0.view(L, blocks, D // blocks).transpose(0, 1).contiguous()
                                lib.headnorm_rope_blocked_(q, k, *args, round_mode=rm, q_out_scale=qs)
                                emit(f"headnorm_rope_blocked {name}", q, k)


def run_quant():
    for K in DS:
        for M in MS:
            x = rows(M, K)
            emit(f"quant_fp8_rowwise K={K} M={M}", *lib.quant_fp8_rowwise(x))
            emit(f"quant_int8_rowwise K={K} M={M}", *lib.quant_int8_rowwise(x))
            if K % 16 == 0:
                xb = x.view(M, 2, K // 2).transpose(0, 1).contiguous()  # K-blocked [2, M, K / 2]
                emit(f"quant_fp8_rowwise_blocked K={K} M={M}", *lib.quant_fp8_rowwise(xb))
                emit(f"quant_int8_rowwise_blocked K={K} M={M}", *lib.quant_int8_rowwise(xb))


def run_elementwise():
    for D in (8, 520, 5120):
        for M in MS:
            x, y, g = rows(M, D), rows(M, D), rand(D)
            emit(f"gate_residual gate D={D} M={M}", lib.gate_residual_(x.clone(), y, g))
            emit(f"gate_residual D={D} M={M}", lib.gate_residual_(x.clone(), y))
    x = rows(37, 8192).view(-1)[: 37 * 8192 - 3] * 0.01  # the outlier scaled into the activations' range; a tail of 5 elements
    for act in (lib.EPI_GELU_TANH, lib.EPI_SILU, lib.ACT_GELU_ERF):
        emit(f"activation act={act}", lib.activation(x.contiguous(), act))
    emit("sinusoid_embed", lib.sinusoid_embed(torch.tensor([0, 1, 500, 999], device="cuda"), 256))


def run_thin_entries():
    """the entries that only forward to the ones above, through the C ABI"""
    M, D, H = 37, 1536, 12
    x, sc, sh, y = rows(M, D), rand(D, scale=0.1), rand(D, scale=0.1), torch.zeros(M, D, dtype=BF16, device="cuda")
    p = lib._p
    lib._check(lib._lib.x2v_layernorm_bf16(p(x), D, None, None, p(sc), p(sh), p(y), D, M, D, 1e-6, None), "layernorm")
    emit("x2v_layernorm_bf16", y)
    cs, wq, wk = rope_table(), rand(D), rand(D)
    q, k = rows(M, D), rows(M, D)
    lib._check(lib._lib.x2v_rmsnorm_rope_bf16(p(q), D, p(k), D, p(wq), p(wk), p(cs), M, H, 0, 2, 3, 5, 1e-6, lib.ROUND_FP32, None), "rmsnorm_rope")
    emit("x2v_rmsnorm_rope_bf16", q, k)
    lib._check(lib._lib.x2v_rmsnorm_rope_scaled_bf16(p(q), D, p(k), D, p(wq), p(wk), p(cs), M, H, 0, 2, 3, 5, 1e-6, lib.ROUND_REF, 0.1275, None), "rmsnorm_rope")
    emit("x2v_rmsnorm_rope_scaled_bf16", q, k)
    xq, s = torch.zeros(M, D, dtype=torch.uint8, device="cuda"), torch.zeros(M, dtype=torch.float32, device="cuda")
    lib._check(lib._lib.x2v_quant_fp8_rowwise(p(x), D, p(xq), D, p(s), M, D, None), "quant_fp8")
    emit("x2v_quant_fp8_rowwise", xq, s)
    lib._check(lib._lib.x2v_quant_int8_rowwise(p(x), D, p(xq), D, p(s), M, D, None), "quant_int8")
    emit("x2v_quant_int8_rowwise", xq, s)


if __name__ == "__main__":
    lib.init(0)
    print(f"# {lib.LIB_PATH}: {lib.version()}")
    run_rmsnorm()
    run_layernorm()
    run_rmsnorm_rope()
    run_headnorm_rope()
    run_quant()
    run_elementwise()
    run_thin_entries()
