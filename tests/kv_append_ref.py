"""x2v_transpose_heads_append_bf16 restated in NumPy on uint16 bit patterns (the append is a bit copy, so no bf16 arithmetic is involved), the
whole-sequence transpose from the layout formula of include/x2v.h, and the checker that tests/test_gpu_kv_append.py applies to the kernel's
output.  tests/test_kv_append_host.py shows that the checker rejects six plausible wrong appends."""
import numpy as np

D, KV = 128, 64  # head dim, keys per V^T tile


def vt_offset(h, key, dv, ldvt):
    """include/x2v.h: element (head h, key, component dv) of V^T [H][ldvt/64][128][64]."""
    return ((h * (ldvt // KV) + key // KV) * D + dv) * KV + key % KV


def transpose_ref(v, H, ldvt=None):
    """x2v_transpose_heads_bf16: v [Sk, >= H*128] uint16 -> V^T [H, ldvt/64, 128, 64] with keys >= Sk zero — element by element from vt_offset."""
    Sk = v.shape[0]
    ldvt = (Sk + KV - 1) // KV * KV if ldvt is None else ldvt
    flat = np.zeros(H * ldvt * D, dtype=np.uint16)
    h, key, dv = np.meshgrid(np.arange(H), np.arange(Sk), np.arange(D), indexing="ij")
    flat[vt_offset(h, key, dv, ldvt)] = v[key, h * D + dv]
    return flat.reshape(H, ldvt // KV, D, KV)


def append_ref(vt, v, key0):
    """The contract: a copy of vt [H, tiles, 128, 64] in which key key0 + s of head h, component dv is v[s, h*128 + dv]; nothing else changed."""
    H, tiles = vt.shape[:2]
    S = v.shape[0]
    assert 0 <= key0 and key0 + S <= tiles * KV
    out = vt.copy().reshape(-1)
    if S:
        h, s, dv = np.meshgrid(np.arange(H), np.arange(S), np.arange(D), indexing="ij")
        out[vt_offset(h, key0 + s, dv, tiles * KV)] = v[s, h * D + dv]
    return out.reshape(vt.shape)


def check_append(before, after, v, key0):
    """What the GPU test asserts of the kernel's result `after` (all uint16 arrays; before / after [H, tiles, 128, 64], v [S, >= H*128]):
    the touched range is bit-equal to v, every other element is bit-equal to `before`.  Raises AssertionError naming the first difference."""
    H, tiles = before.shape[:2]
    S = v.shape[0]
    assert after.shape == before.shape and after.dtype == before.dtype == np.uint16
    keys = np.arange(tiles * KV)
    # [H, keys, dv] views of both caches
    a = after.transpose(0, 1, 3, 2).reshape(H, tiles * KV, D)
    b = before.transpose(0, 1, 3, 2).reshape(H, tiles * KV, D)
    inside = (keys >= key0) & (keys < key0 + S)
    want = v[:, : H * D].reshape(S, H, D).transpose(1, 0, 2)
    got = a[:, inside]
    if not np.array_equal(got, want):
        h, s, dv = (int(i[0]) for i in np.nonzero(got != want))
        raise AssertionError(f"touched range: head {h} key {key0 + s} dv {dv} holds {got[h, s, dv]:#06x}, v has {want[h, s, dv]:#06x}")
    if not np.array_equal(a[:, ~inside], b[:, ~inside]):
        h, k, dv = (int(i[0]) for i in np.nonzero(a[:, ~inside] != b[:, ~inside]))
        key = int(keys[~inside][k])
        raise AssertionError(f"outside [{key0}, {key0 + S}): head {h} key {key} dv {dv} changed from {b[h, key, dv]:#06x} to {a[h, key, dv]:#06x}")


def cache_pattern(H, tiles):
    """A position-dependent, finite, non-zero bf16 bit pattern for a cache [H, tiles, 128, 64]: exponent field 121 or 123 (|x| in [2^-6, 2^-3)), the rest
    from the element's index, so that no two neighbouring elements, tiles or heads agree."""
    i = np.arange(H * tiles * D * KV, dtype=np.uint64)
    mant = (i * np.uint64(2654435761) >> np.uint64(7)) & np.uint64(0x01FF)
    sign = (i >> np.uint64(3)) & np.uint64(1)
    return ((sign << np.uint64(15)) | np.uint64(0x3C00) | mant | np.uint64(0x0080)).astype(np.uint16).reshape(H, tiles, D, KV)


def v_pattern(S, H, seed=1):
    """A finite bf16 bit pattern [S, H*128] distinct from cache_pattern (exponent field 128 or 129: |x| in [2, 8))."""
    s, c = np.meshgrid(np.arange(S, dtype=np.uint64), np.arange(H * D, dtype=np.uint64), indexing="ij")
    i = s * np.uint64(H * D) + c + np.uint64(seed) * np.uint64(7919)
    mant = (i * np.uint64(40503) >> np.uint64(3)) & np.uint64(0x00FF)
    sign = (i >> np.uint64(5)) & np.uint64(1)
    return ((sign << np.uint64(15)) | np.uint64(0x4000) | mant).astype(np.uint16)


# ---- plausible wrong appends: each must be rejected by check_append (tests/test_kv_append_host.py) ----
def wrong_shifted(vt, v, key0):
    """off by one key"""
    return append_ref(vt, v, key0 + 1)


def wrong_first_tile_zeroed(vt, v, key0):
    """the whole-sequence kernel's habit: the keys of the first tile in front of key0 zero-filled"""
    out = append_ref(vt, v, key0)
    out[:, key0 // KV, :, : key0 % KV] = 0
    return out


def wrong_tail_zeroed(vt, v, key0):
    """the whole-sequence kernel's zero fill behind the last key, up to the tile's end"""
    out = append_ref(vt, v, key0)
    end = key0 + v.shape[0]
    if end % KV:
        out[:, end // KV, :, end % KV :] = 0
    return out


def wrong_heads_swapped(vt, v, key0):
    H = vt.shape[0]
    perm = np.concatenate([np.arange(1, H), [0]])
    return append_ref(vt, v[:, : H * D].reshape(-1, H, D)[:, perm].reshape(-1, H * D), key0)


def wrong_tile_transposed(vt, v, key0):
    """a tile written [key][dv] instead of [dv][key]: within each 64-key tile, (dv, key) -> the flat position key * 128 + dv"""
    H, tiles = vt.shape[:2]
    out = vt.copy().reshape(H, tiles, D * KV)
    for s in range(v.shape[0]):
        key = key0 + s
        for h in range(H):
            out[h, key // KV, (key % KV) * D + np.arange(D)] = v[s, h * D : (h + 1) * D]
    return out.reshape(vt.shape)


def wrong_word_granular(vt, v, key0):
    """a writer that only knows 16-byte words (8 keys): a word that straddles an end of the range is stored whole, its out-of-range keys zero"""
    out = append_ref(vt, v, key0)
    end = key0 + v.shape[0]
    lo, hi = key0 // 8 * 8, (end + 7) // 8 * 8
    for key in list(range(lo, key0)) + list(range(end, hi)):
        out[:, key // KV, :, key % KV] = 0
    return out


WRONG_APPENDS = [wrong_shifted, wrong_first_tile_zeroed, wrong_tail_zeroed, wrong_heads_swapped, wrong_tile_transposed, wrong_word_granular]
