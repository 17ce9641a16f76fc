"""Radial attention's static block mask (host side, CPU-capable).

`MaskMap(video_token_num, num_frame).queryLogMask(query, "radial", block_size=128, decay_factor=..., model_type="wan" | "hunyuan")` returns the
bool [n, n] mask of 128 x 128 (query rows x keys) blocks, n = query.shape[0] // 128, that the reference's RadialAttnWeight hands to its block-sparse
attention (attentions/common/radial_attn.py:197-211 -> gen_log_mask_shrinked :154-194) — bit for bit, which tests/golden/radial_masks.npz pins.

The reference paints, for every pair of frames (i, j), a dense [tokens per frame]^2 token mask — a band |c - r| <= window(|i - j|), or everything for
the first key frame (the attention sink), or nothing for the frame distances its split rule drops — pads it to whole blocks from where the two frames
start inside their first blocks, and keeps a block when more than 0.6 of its non-empty key columns are more than 1/3 full.  A band is an interval
per column, so the number of attended rows of a block in a column is an interval intersection: this module computes those counts directly, one
[blocks, columns] integer table per frame pair, and applies the same two thresholds.  What follows from the reference's arithmetic and is kept:

  * the padded frame-pair mask is cut to ceil(tpf / 128) blocks on BOTH axes, counted from the block the frame starts in: the tokens of a frame
    that spill into one more block (a frame that does not start on a block boundary) do not vote, on the row side and on the column side alike;
  * rows and columns are not symmetric: the density is taken along a block's rows per key column, so block (a, b) and block (b, a) differ;
  * everything from block video_token_num // 128 on (the partial last block, or text tokens) is dense in both directions, and the blocks below
    that border come from the frame pairs alone;
  * "wan" attends half a frame (tpf // 2) at frame distance 1, "hunyuan" the whole frame; from distance 2 on the window is
    2^bit_length(tpf) / 2^bit_length(dist) * decay_factor, never below 128, and a distance is dropped altogether when 128 / (2^bit_length(tpf) /
    2^bit_length(dist)) (truncated) does not divide it;
  * the thresholds are float32 comparisons of count / 128 with 1/3 and of full / (nonempty + 1e-9) with 0.6, done here by the same tensor
    operations on the counts.
"""
import torch

BLOCK = 128


def _window(dist, tpf, decay_factor, model_type):
    """Half-width of the band at frame distance `dist` (tokens; may be fractional) and whether the distance is attended at all."""
    if model_type not in ("wan", "hunyuan"):
        raise ValueError(f"Unknown model type: {model_type}")
    span = 2 ** tpf.bit_length() / 2 ** dist.bit_length()
    keep = span >= BLOCK or dist % int(BLOCK / span) == 0
    if dist == 0 or (dist == 1 and model_type == "hunyuan"):
        return tpf, keep
    if dist == 1:
        return tpf // 2, keep
    return max(span * decay_factor, BLOCK), keep


def _pair_blocks(tpf, row0, col0, width, nb, rows_v, cols_v):
    """[nb, nb] bool: which blocks of the frame pair's padded mask survive the density rule.  row0 / col0: where the frames start inside their first
    blocks; width: band half-width (>= tpf: everything).  rows_v [nb, 1] = 128 * block, cols_v [1, nb * 128] = padded column."""
    edge = nb * BLOCK
    w = min(int(width), tpf)  # |c - r| <= width over integers
    lo_b = torch.clamp(rows_v, min=row0)
    hi_b = torch.clamp(rows_v + BLOCK, max=min(row0 + tpf, edge))
    diag = cols_v - col0 + row0  # the padded row on the diagonal of this column
    cnt = torch.clamp(torch.minimum(hi_b, diag + w + 1) - torch.maximum(lo_b, diag - w), min=0)
    cnt = cnt * ((cols_v >= col0) & (cols_v < min(col0 + tpf, edge)))
    dens = (cnt / BLOCK).view(nb, nb, BLOCK)
    full = (dens > 1 / 3).sum(dim=-1)
    nonempty = (dens > 0).sum(dim=-1)
    return full / (nonempty + 1e-9) > 0.6


def radial_block_mask(n_blocks, video_token_num, num_frame, decay_factor, model_type):
    """The mask below the border (see the module text), as the reference generates it for a sequence of n_blocks * 128 rows."""
    tpf = video_token_num // num_frame
    border = video_token_num // BLOCK
    nb = (tpf - 1) // BLOCK + 1
    out = torch.zeros((n_blocks, n_blocks), dtype=torch.bool)
    out[border:] = True
    out[:, border:] = True
    rows_v = (torch.arange(nb, dtype=torch.int64) * BLOCK).view(nb, 1)
    cols_v = torch.arange(nb * BLOCK, dtype=torch.int64).view(1, nb * BLOCK)
    cache = {}
    for i in range(num_frame):
        for j in range(num_frame):
            width, keep = (tpf, True) if j == 0 else _window(abs(i - j), tpf, decay_factor, model_type)
            if not keep:
                continue
            row0, col0 = (i * tpf) % BLOCK, (j * tpf) % BLOCK
            key = (row0, col0, int(width))
            if key not in cache:
                cache[key] = _pair_blocks(tpf, row0, col0, width, nb, rows_v, cols_v)
            r, c = (i * tpf) // BLOCK, (j * tpf) // BLOCK
            if r + nb > n_blocks or c + nb > n_blocks:
                raise ValueError(f"radial mask: frame pair ({i}, {j}) does not fit {n_blocks} blocks (the query must be padded to whole blocks)")
            out[r : r + nb, c : c + nb] |= cache[key]
    return out


class MaskMap:
    def __init__(self, video_token_num=79200, num_frame=22):
        self.video_token_num = video_token_num
        self.num_frame = num_frame
        self.log_mask = None

    def queryLogMask(self, query, sparse_type, block_size=128, decay_factor=0.5, model_type=None):
        if sparse_type != "radial":
            raise ValueError(f"MaskMap: sparse_type {sparse_type!r} (only 'radial')")
        if block_size != BLOCK:
            raise ValueError(f"MaskMap: block_size {block_size} (only {BLOCK} is built)")
        n = query.shape[0] // BLOCK
        if self.log_mask is None:  # cached for the object's lifetime, as in the reference: later calls ignore decay_factor / model_type
            self.log_mask = radial_block_mask(n, self.video_token_num, self.num_frame, decay_factor, model_type)
        bound = self.video_token_num // BLOCK
        log_mask = torch.ones((n, n), dtype=torch.bool)
        log_mask[:bound, :bound] = self.log_mask[:bound, :bound]
        device = getattr(query, "device", None)
        return log_mask if device is None else log_mask.to(device)
