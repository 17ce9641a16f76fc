"""Host-side checks of the V^T cache append (x2v_transpose_heads_append_bf16): its NumPy restatement against the layout formula of
include/x2v.h, the GPU test's checker against six plausible wrong appends, and the entry's argument validation, which runs before any GPU call."""
import ctypes

import numpy as np
import pytest

from tests.kv_append_ref import KV, WRONG_APPENDS, append_ref, cache_pattern, check_append, transpose_ref, v_pattern

OK, E_SHAPE, E_ALIGN, E_ARG = 0, -1, -2, -5  # include/x2v.h


@pytest.mark.parametrize("H", [1, 3])
def test_appends_in_order_into_a_zeroed_cache_are_the_whole_sequence_transpose(H):
    """Four blocks of 45 rows (first-tile remainders 0, 45, 26, 7) into a zeroed cache of 192 keys: the layout of x2v_transpose_heads_bf16 over the
    180 concatenated rows, taken from the layout formula — zero tail included."""
    v = v_pattern(180, H)
    vt = np.zeros((H, 3, 128, 64), dtype=np.uint16)
    for j in range(4):
        vt = append_ref(vt, v[45 * j : 45 * j + 45], 45 * j)
    assert np.array_equal(vt, transpose_ref(v, H, 192))
    # and with a token stride longer than H*128 (columns behind the heads are never looked at)
    wide = np.full((180, H * 128 + 8), 0x7FC0, dtype=np.uint16)
    wide[:, : H * 128] = v
    assert np.array_equal(append_ref(np.zeros_like(vt), wide, 0), transpose_ref(v, H, 192))


def test_checker_accepts_the_contract_and_rejects_six_wrong_appends():
    H, key0, S = 3, 45, 45  # odd start, crosses a tile boundary, ends mid-tile and mid-word; one spare tile behind
    before, v = cache_pattern(H, 3), v_pattern(S, H)
    check_append(before, append_ref(before, v, key0), v, key0)
    assert len(WRONG_APPENDS) == 6
    for wrong in WRONG_APPENDS:
        after = wrong(before, v, key0)
        with pytest.raises(AssertionError):
            check_append(before, after, v, key0)
    # each wrong append is wrong in its own region: the message says where
    with pytest.raises(AssertionError, match="outside"):
        check_append(before, WRONG_APPENDS[1](before, v, key0), v, key0)  # first-tile remainder
    with pytest.raises(AssertionError, match="outside"):
        check_append(before, WRONG_APPENDS[5](before, v, key0), v, key0)  # the straddling 16-byte words
    with pytest.raises(AssertionError, match="touched range"):
        check_append(before, WRONG_APPENDS[3](before, v, key0), v, key0)  # heads


def test_checker_sees_a_single_changed_element_anywhere():
    H, key0, S = 2, 7, 60
    before, v = cache_pattern(H, 3), v_pattern(S, H)
    good = append_ref(before, v, key0)
    for h, t, dv, kk in [(0, 0, 0, 6), (1, 1, 127, 3), (0, 2, 5, 63), (1, 0, 64, 7), (0, 1, 9, 2)]:  # both edges, a spare tile, both sides of each boundary
        bad = good.copy()
        bad[h, t, dv, kk] ^= 1
        with pytest.raises(AssertionError):
            check_append(before, bad, v, key0)


def test_argument_validation_needs_no_gpu():
    """Every check of the entry, in the order the header gives them; none reaches a GPU call.  Fails on a library without the entry."""
    from lightx2v_amd import lib

    f = lib._lib.x2v_transpose_heads_append_bf16
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)
    err = lambda: lib._lib.x2v_last_error()  # noqa: E731
    # (v, ldv, vt, ldvt, key0, S, H, stream)
    assert f(None, 128, a, 64, 0, 8, 1, None) == E_ARG and err().startswith(b"transpose_heads_append:")
    assert f(a, 128, None, 64, 0, 8, 1, None) == E_ARG
    for ldvt, key0, S, H in [(63, 0, 8, 1), (100, 0, 8, 1), (64, -1, 8, 1), (64, 0, -1, 1), (64, 60, 5, 1), (64, 65, 0, 1), (128, 64, 65, 1), (64, 0, 8, 0), (64, 0, 8, -3),
                             (64, 0, 8, 65536)]:
        assert f(a, 128 * max(H, 1), a, ldvt, key0, S, H, None) == E_SHAPE, (ldvt, key0, S, H)
        assert err().startswith(b"transpose_heads_append:")
    assert f(a, 128, a, 1 << 62, (1 << 62) - 4, 1 << 62, 1, None) == E_SHAPE  # key0 + S overflows int64: still refused
    assert f(odd, 128, a, 64, 0, 8, 1, None) == E_ALIGN and err().startswith(b"transpose_heads_append:")
    assert f(a, 128, odd, 64, 0, 8, 1, None) == E_ALIGN
    assert f(a, 132, a, 64, 0, 8, 1, None) == E_ALIGN  # ldv % 8
    assert f(a, 128, a, 64, 0, 8, 2, None) == E_SHAPE  # token stride shorter than H*128
    # no rows: nothing launched, whatever the (valid) offset
    assert f(a, 128, a, 64, 0, 0, 1, None) == OK
    assert f(a, 128, a, 128, 64 + 7, 0, 3 * 0 + 1, None) == OK
    assert f(a, 128, a, 64, 64, 0, 1, None) == OK  # key0 == ldvt with S == 0 is inside the cache


def test_python_wrappers_fail_loudly_without_a_gpu_tensor():
    import torch

    from lightx2v_amd import lib

    v = torch.zeros(8, 128, dtype=torch.bfloat16)
    vt = torch.zeros(1, 1, 128, 64, dtype=torch.bfloat16)
    with pytest.raises(lib.X2VError):
        lib.transpose_heads_append(v, vt, 0)
    with pytest.raises(lib.X2VError):
        lib.attention_cached(v, v, vt, 8, 1)
    assert KV == 64
