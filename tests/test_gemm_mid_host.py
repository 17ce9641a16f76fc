"""x2v_gemm_mid_f16, host side (no GPU): the entry's argument checks, and the workspace size and the tile / split choice as host arithmetic."""
import ctypes

import pytest

from lightx2v_amd import lib

KT = 64  # K elements per K tile
SLOT = 128 * 128 * 4  # bytes of one fp32 partial tile


def test_gemm_mid_abi_argument_validation_needs_no_gpu():
    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)
    # x2v_gemm_mid_f16(x, ldx, w, ldw, bias, y, ldy, M, N, K, epilogue, resid, ldr, splits, workspace, workspace_bytes, stream)
    tail = (0, None, 0, None)
    assert L.x2v_gemm_mid_f16(None, 64, a, 64, None, a, 64, 4, 64, 64, 0, None, 0, *tail) == -5
    assert L.x2v_gemm_mid_f16(a, 600, a, 600, None, a, 64, 4, 64, 588, 0, None, 0, *tail) == -1  # K % 32
    assert b"K=588" in L.x2v_last_error()
    assert L.x2v_gemm_mid_f16(a, 64, a, 64, None, a, 64, 4, 60, 64, 0, None, 0, *tail) == -1  # N % 8
    assert b"N=60" in L.x2v_last_error()
    assert L.x2v_gemm_mid_f16(a, 64, a, 64, None, a, 64, 4097, 64, 64, 0, None, 0, *tail) == -1  # M beyond the mid-M form
    for epi in (1, 3, 5):  # GELU, quick-GELU, unknown
        assert L.x2v_gemm_mid_f16(a, 64, a, 64, a, a, 64, 4, 64, 64, epi, None, 0, *tail) == -5
    assert L.x2v_gemm_mid_f16(a, 64, a, 64, None, a, 64, 4, 64, 64, 2, None, 0, *tail) == -5  # residual epilogue without resid
    assert L.x2v_gemm_mid_f16(a, 64, a, 64, a, a, 64, 4, 64, 64, 4, None, 0, *tail) == -5  # SwiGLU with a bias
    assert L.x2v_gemm_mid_f16(a, 60, a, 64, None, a, 64, 4, 64, 64, 0, None, 0, *tail) == -2  # ldx < K
    assert L.x2v_gemm_mid_f16(odd, 64, a, 64, None, a, 64, 4, 64, 64, 0, None, 0, *tail) == -2  # alignment
    assert L.x2v_gemm_mid_f16(a, 64, a, 64, None, a, 64, 0, 64, 64, 0, None, 0, *tail) == 0  # no rows: nothing launched
    # the split arguments: more splits than K tiles, no workspace, a workspace one byte short
    assert L.x2v_gemm_mid_f16(a, 128, a, 128, None, a, 64, 4, 64, 128, 0, None, 0, 3, a, 1 << 30, None) == -5
    assert b"splits=3" in L.x2v_last_error()
    need = L.x2v_gemm_mid_workspace_bytes(351, 4096, 4096, 3)
    assert L.x2v_gemm_mid_f16(a, 4096, a, 4096, None, a, 4096, 351, 4096, 4096, 0, None, 0, 3, None, 0, None) == -5
    assert L.x2v_gemm_mid_f16(a, 4096, a, 4096, None, a, 4096, 351, 4096, 4096, 0, None, 0, 3, a, need - 1, None) == -5
    assert str(need).encode() in L.x2v_last_error()
    assert L.x2v_gemm_mid_f16(a, 128, a, 128, None, a, 16384, 4096, 16384, 128, 0, None, 0, 2, a, 1 << 40, None) == -5  # more tiles than counters
    assert b"4096 output tiles" in L.x2v_last_error()


def test_gemm_mid_workspace_bytes_is_host_arithmetic():
    L = lib._lib
    assert L.x2v_gemm_mid_workspace_bytes(351, 4096, 4096, 1) == 0
    assert L.x2v_gemm_mid_workspace_bytes(351, 4096, 4096, 3) == 4096 + 96 * 3 * SLOT  # 1024 counters whatever the shape, then 3 x 32 tiles x 3 slots
    assert L.x2v_gemm_mid_workspace_bytes(127, 136, 2080, 2) == 4096 + 2 * 2 * SLOT
    assert L.x2v_gemm_mid_workspace_bytes(0, 136, 2080, 2) == 0


@pytest.mark.parametrize("M, N, K, cus, splits", [
    (351, 28672, 4096, 256, 1),   # gate | up: 3 x 224 tiles fill the machine
    (256, 16384, 4096, 256, 1),   # exactly cu_count tiles
    (351, 6144, 4096, 256, 2),    # q | k | v: 144 tiles
    (351, 4096, 4096, 256, 3),    # o: 96 tiles
    (351, 4096, 14336, 256, 3),   # down
    (351, 136, 2080, 256, 16),    # 6 tiles: capped at 16 and at half of the 33 K tiles
    (129, 256, 512, 256, 4),      # 8 K tiles: ranges of at least two
    (130, 256, 64, 256, 1),       # one K tile cannot be split
    (351, 4096, 4096, 64, 1),
])
def test_gemm_mid_choice_is_host_arithmetic(M, N, K, cus, splits):
    assert lib.gemm_mid_choice(M, N, K, cus) == ((128, 128), splits)
    assert splits <= (K + KT - 1) // KT
    assert lib._lib.x2v_gemm_mid_choice(0, N, K, cus) == -1 and lib._lib.x2v_gemm_mid_choice(M, N, K, 0) == -1
