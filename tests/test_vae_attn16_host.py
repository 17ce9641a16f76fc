"""Argument validation of the fused VAE attention entries (x2v_vae_attn_prep_f16, x2v_vae_attn_f16) runs before any HIP call: no GPU needed."""
import ctypes

import pytest


@pytest.mark.parametrize("entry", ["prep", "attn"])
def test_vae_attn16_argument_validation(entry):
    from lightx2v_amd import lib

    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)
    if entry == "prep":  # (qkv, ld, q16, k16, vt16, n, C, stream)
        call = lambda C=512, p=a, n=72: L.x2v_vae_attn_prep_f16(p, 3 * C, a, a, a, n, C, None)  # noqa: E731
        assert call(n=0) == -1
    else:  # (q16, k16, vt16, out, ldo, frames, hw, C, scale, stream)
        call = lambda C=512, p=a, frames=3, hw=24: L.x2v_vae_attn_f16(a, p, a, a, C, frames, hw, C, 0.05, None)  # noqa: E731
        assert call(hw=0) == -1 and call(frames=0) == -1
    assert call(C=384) == -1  # the Wan VAE's width is not built
    assert b"384" in L.x2v_last_error()
    assert call(p=None) == -5
    assert call(p=odd) == -2
