"""Wan CausVid — the reference's autoregressive Wan (`wan2.1_causvid`) on the HIP kernels.  Host-side mirror of
lightx2v/models/runners/wan/wan_causvid_runner.py, models/networks/wan/causvid_model.py and models/networks/wan/infer/causvid/transformer_infer.py:
the video is generated in blocks of `num_frame_per_block` latent frames, a block's queries attend the keys of all earlier blocks plus its own, and
every denoise step of a block rewrites that block's K and V in a per-layer cache at token offset `kv_start`.

The reference keeps K and V row-major and lets flash-attention read them in place.  The self-attention kernel here reads V as
V^T [H][tiles][128][64], so the cache holds K row-major and V ONLY as V^T, and a block's v rows go into it with lib.transpose_heads_append — at
offsets that are no multiple of the 64-key tile (4680 % 64 = 8 at 480p).  Everything else is the dense driver's: the norm + RoPE kernel takes
`kv_start` as its global token offset, attention runs with Sq != Sk, cross-attention and FFN are WanTransformerInfer's, and its step-invariant
cross-attention K / V cache plays the reference's `crossattn_cache`.

Not built (NotImplementedError where met): `num_fragments > 1` (the reference's fragment path reads `scheduler.last_sample`, which its step-distill
scheduler never sets), parallel attention (the reference raises there too), CFG, radial and block-scaled fp8 self-attention."""
import inspect

import torch

from . import lib
from .wan import WanModel, WanTransformerInfer, _cfg


class KVCache:
    """The self-attention cache of `num_layers` blocks for `capacity` tokens: per layer k [capacity, H*128] row-major and
    vt [H, ceil(capacity/64), 128, 64], both bf16 and zero-filled ONCE (the reference's `_init_kv_cache`: zeros of num_frames * frame_seq_length
    rows).  There is no row-major V.  The zero fill is what keeps every byte behind the keys in use finite, which lib.attention_cached needs; after
    it nothing but the k projection's `out=`, the in-place norm + RoPE and lib.transpose_heads_append write here, all on the caller's stream."""

    def __init__(self, num_layers, capacity, num_heads, device):
        self.capacity, self.num_heads = int(capacity), int(num_heads)
        tiles = (self.capacity + 63) // 64
        self.layers = [
            {"k": torch.zeros((self.capacity, num_heads * 128), dtype=torch.bfloat16, device=device),
             "vt": torch.zeros((num_heads, tiles, 128, 64), dtype=torch.bfloat16, device=device)}
            for _ in range(num_layers)
        ]

    def __getitem__(self, layer):
        return self.layers[layer]

    def __len__(self):
        return len(self.layers)


class WanTransformerInferCausVid(WanTransformerInfer):
    """reference: wan/infer/causvid/transformer_infer.py:8-220 (no-offload path)."""

    def __init__(self, config):
        super().__init__(config)
        self.num_frames = _cfg(config, "num_frames")
        self.num_frame_per_block = _cfg(config, "num_frame_per_block")
        self.frame_seq_length = _cfg(config, "frame_seq_length")
        self.kv_cache = None
        self._kv = None  # (layer cache, kv_start, kv_end) of the block in flight

    def _init_kv_cache(self, capacity=None, device="cuda"):
        """transformer_infer.py:18-30; `capacity` defaults to num_frames * frame_seq_length tokens."""
        self.kv_cache = KVCache(self.blocks_num, self.num_frames * self.frame_seq_length if capacity is None else capacity, self.num_heads, device)
        return self.kv_cache

    def _init_crossattn_cache(self):
        """transformer_infer.py:32-44: the parent's step-invariant `_cross_kv` cache is the cross-attention cache; a new video starts it empty."""
        self.clear_cross_kv()

    def infer(self, weights, grid_sizes, embed, x, embed0, seq_lens, freqs, context, kv_start, kv_end):
        self._refuse_unbuilt_causvid(weights)
        if self.kv_cache is None:
            raise lib.X2VError("causvid: no KV cache (call _init_kv_cache, as the runner does)")
        if not (0 <= kv_start < kv_end <= self.kv_cache.capacity) or x.shape[0] != kv_end - kv_start:
            raise lib.X2VError(f"causvid: kv_start={kv_start} kv_end={kv_end} do not frame the block's {x.shape[0]} tokens inside a cache of {self.kv_cache.capacity}")
        try:
            for block_idx in range(self.blocks_num):
                self._kv = (self.kv_cache[block_idx], int(kv_start), int(kv_end))
                x = self.infer_block(weights.blocks[block_idx], grid_sizes, embed, x, embed0, seq_lens, freqs, context)
        finally:
            self._kv = None
        return x

    def _refuse_unbuilt_causvid(self, weights):
        """Per call, as the parent's check: these are plain attributes that a caller may set on a live object."""
        if self.parallel_attention is not None:
            raise NotImplementedError("wan2.1_causvid with parallel attention (parallel_attn_type): not built, and the reference raises here too")
        if self._pair is not None:
            raise NotImplementedError("wan2.1_causvid in the CFG pair pass: the causal driver runs one conditional forward per step (enable_cfg is false in the reference's configs)")
        if self.radial:
            raise NotImplementedError("wan2.1_causvid with self_attn_1_type='hip_radial': the block-sparse kernel runs one whole sequence per launch, not a KV cache")
        if self.mx_attn:
            raise NotImplementedError("wan2.1_causvid with self_attn_1_type='hip_mxfp8': the block-scaled fp8 kernel has no quantised KV cache")
        op = weights.blocks[0].compute_phases[1].self_attn_k
        if "out" not in inspect.signature(op.apply).parameters:
            raise NotImplementedError(f"wan2.1_causvid with mm_type operator class {type(op).__name__}: its apply() has no out=, which the k projection into the cache needs")

    def _self_attn_route(self, weights, x):
        return "causvid" if self._kv is not None else super()._self_attn_route(weights, x)

    def _self_attn_causvid(self, weights, x, n1, mmkw, freqs, grid, fast, variant, rope_args):
        """transformer_infer.py:94-136 up to the attention: k into the cache rows of this block, norm + RoPE in place at the block's frame offset,
        v appended to V^T, attention of the block's queries over keys [0, kv_end).  Both rounding modes attend through the V^T kernel; q is prescaled
        exactly when the dense driver prescales it."""
        cache, kv_start, kv_end = self._kv
        k_rows = cache["k"][kv_start:kv_end]
        v = weights.self_attn_v.apply(n1, **mmkw)  # row-major: the epilogue V^T form writes whole zero-filled tiles from key 0
        q = weights.self_attn_q.apply(n1, **mmkw)
        weights.self_attn_k.apply(n1, out=k_rows, **mmkw)
        gh, gw = grid[1], grid[2]
        if kv_start % (gh * gw) or kv_end % (gh * gw):
            raise lib.X2VError(f"causvid: kv_start={kv_start} / kv_end={kv_end} are not whole frames of {gh}x{gw} tokens")
        # compute_freqs_causvid(..., start_frame = kv_start // (gh*gw)): the kernel's global token offset, on a grid that reaches the block's last frame
        rope = dict(rope_args, s0=kv_start)
        lib.rmsnorm_rope_(q, k_rows, weights.self_attn_norm_q.weight, weights.self_attn_norm_k.weight, freqs, (kv_end // (gh * gw), gh, gw), self.num_heads, **rope)
        lib.transpose_heads_append(v, cache["vt"], kv_start)
        return self._timed("self", lambda: lib.attention_cached(q, cache["k"], cache["vt"], kv_end, self.num_heads, prescaled=fast))


class WanCausVidModel(WanModel):
    """reference: wan/causvid_model.py:18-62."""

    def _init_infer_class(self):
        super()._init_infer_class()
        if self.transformer_infer_class is not WanTransformerInfer:
            raise NotImplementedError(f"wan2.1_causvid with feature_caching={_cfg(self.config, 'feature_caching')}: not built")
        self.transformer_infer_class = WanTransformerInferCausVid

    def init_kv_cache(self, capacity=None):
        """What the runner's run() does first (wan_causvid_runner.py:76-77)."""
        self.transformer_infer._init_crossattn_cache()
        return self.transformer_infer._init_kv_cache(capacity, self.device)

    @torch.no_grad()
    def infer(self, inputs, kv_start, kv_end):
        if _cfg(self.config, "enable_cfg", False):
            raise NotImplementedError("wan2.1_causvid with enable_cfg: the causal driver runs one conditional forward per step (CFG, and its pair pass, are not built; the reference's configs disable it)")
        embed, grid_sizes, pre_infer_out = self.pre_infer.infer(self.pre_weight, inputs, positive=True, kv_start=kv_start, kv_end=kv_end)
        x = self.transformer_infer.infer(self.transformer_weights, grid_sizes, embed, *pre_infer_out, kv_start, kv_end)
        self.scheduler.noise_pred = self.post_infer.infer(self.post_weight, x, embed, grid_sizes)[0]


def causvid_plan(config):
    """(frame_seq_length, tokens per block, [(kv_start, kv_end) per block], capacity in tokens) of a config — the runner's offset arithmetic
    (wan_causvid_runner.py:90-91,124-125), host-only."""
    ts, ps = config["target_shape"], config["patch_size"]
    nfpb, num_frames, num_blocks = int(config["num_frame_per_block"]), int(config["num_frames"]), int(config["num_blocks"])
    if int(_cfg(config, "num_fragments", 1) or 1) > 1:
        raise NotImplementedError("wan2.1_causvid with num_fragments > 1: the reference's fragment path reads scheduler.last_sample, which its step-distill scheduler never sets")
    if ts[1] != nfpb:
        raise ValueError(f"causvid: target_shape {tuple(ts)} must hold num_frame_per_block={nfpb} latent frames (wan_causvid_runner.py:60-73)")
    fsl = (ts[2] // ps[1]) * (ts[3] // ps[2])
    given = _cfg(config, "frame_seq_length")
    if given is not None and config["task"] == "t2v" and int(given) != fsl:  # i2v: the runner resets it from the input's shape (:63-66)
        raise ValueError(f"causvid: frame_seq_length={given} but a latent frame of {ts[2]}x{ts[3]} has {fsl} tokens")
    if num_blocks < 1 or num_blocks * nfpb > num_frames:
        raise ValueError(f"causvid: num_blocks={num_blocks} x num_frame_per_block={nfpb} exceeds num_frames={num_frames}")
    per_block = nfpb * fsl
    return fsl, per_block, [(b * per_block, (b + 1) * per_block) for b in range(num_blocks)], num_frames * fsl


def run_causvid(model, scheduler, inputs, config, block_latents=None, step_callback=None):
    """reference: wan_causvid_runner.py:75-130 `run()` for num_fragments == 1.  Allocates the caches, then per block: fresh latents, the
    `denoising_step_list` steps of step_pre -> model.infer(inputs, kv_start, kv_end) -> step_post, the block's latents into `output_latents`, the
    offsets advanced by one block.  Returns output_latents [16, num_frames, h, w] bf16 (frames behind num_blocks * num_frame_per_block stay zero, as
    in the reference).

    The reference's step-distill `reset()` redraws the latents (step_distill/scheduler.py:42-43); this project's WanStepDistillScheduler.reset does
    not, so the driver redraws them itself through `scheduler.prepare(latents=...)`: from `block_latents` (a sequence, or a callable block index ->
    tensor [16, num_frame_per_block, h, w]; parity runs inject the fixture's) or else from one generator seeded with config["seed"], one draw per
    block.  `step_callback(block, step)` runs after every step_post."""
    fsl, per_block, offsets, capacity = causvid_plan(config)
    ts = tuple(config["target_shape"])
    nfpb = ts[1]
    if tuple(scheduler.config["target_shape"]) != ts:
        raise ValueError(f"causvid: the scheduler's target_shape {tuple(scheduler.config['target_shape'])} is not the block shape {ts}")
    model.init_kv_cache(capacity)
    gen = None
    output_latents = None
    for block_idx, (kv_start, kv_end) in enumerate(offsets):
        if block_latents is not None:
            lat = block_latents(block_idx) if callable(block_latents) else block_latents[block_idx]
            if tuple(lat.shape) != ts:
                raise ValueError(f"causvid: block {block_idx} latents are {tuple(lat.shape)}, expected {ts}")
        else:
            if gen is None:
                gen = torch.Generator(device=scheduler.device)
                gen.manual_seed(config["seed"])
            lat = torch.randn(*ts, dtype=torch.float32, device=scheduler.device, generator=gen)
        scheduler.prepare(latents=lat)
        scheduler.reset()
        for step_index in range(scheduler.infer_steps):
            scheduler.step_pre(step_index)
            model.infer(inputs, kv_start, kv_end)
            scheduler.step_post()
            if step_callback is not None:
                step_callback(block_idx, step_index)
        if output_latents is None:
            output_latents = torch.zeros((ts[0], int(config["num_frames"]), ts[2], ts[3]), dtype=torch.bfloat16, device=scheduler.latents.device)
        output_latents[:, block_idx * nfpb : (block_idx + 1) * nfpb] = scheduler.latents
    return output_latents
