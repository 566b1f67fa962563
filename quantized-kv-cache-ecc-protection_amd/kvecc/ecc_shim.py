"""ECC-protected paged KV cache shim for HuggingFace models (drop-in).

Mirrors kv_cache/ecc_shim.py of the reference (ECCShimConfig :134-186,
SimpleBlockManager :189-360, ECCBackend :363-1164, ECCPagedAttentionShim
:1167-1392, patch_model_with_ecc_attention :1395-1481, reset_ecc_cache /
get_ecc_stats :1614-1642) with identical cache layout, injection seeds and
statistics, plus the codec-backend selector the reference lacks
(``ECCShimConfig(backend="hip")``).

What changes is how the work is issued.  The reference runs a Python loop
over every (batch, position, kv-head) row with 2 encode + 2 inject Triton
launches and a ``.item()`` per position (ecc_shim.py:626-737), and stacks
cache slices one token at a time in attend (:931-977).  Here a layer's write
is one quantize, one encode, one per-row-seeded injection and one scatter per
K/V tensor (a handful of HIP launches for the whole layer), and attend is one
gather, one decode (+ interpolation) and one dequantization; error counters
accumulate on the device and are read only when asked for (get_ecc_stats).
"""

from __future__ import annotations

import math
from contextlib import contextmanager

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import golay_packed_row_bytes
from .backends import get_codec_backend
from .memory_layout import kv_cache_pair

try:  # optional, as in the reference (:54)
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
except Exception:  # pragma: no cover
    LlamaRotaryEmbedding = None


def compute_injection_seed(base_seed: int, layer_idx: int, injection_count: int) -> int:
    """base_seed + layer_idx*10000 + injection_count (ecc_shim.py:57-80)."""
    return base_seed + layer_idx * 10000 + injection_count


class ECCDummyCache:
    """Placeholder satisfying the transformers cache interface (ecc_shim.py:83-131)."""

    def __init__(self, num_layers=0):
        self.key_cache = []
        self.value_cache = []
        self._num_layers = num_layers
        self._seen_tokens = 0

    def __len__(self):
        return self._num_layers

    def __iter__(self):
        for i in range(len(self.key_cache)):
            yield (self.key_cache[i], self.value_cache[i])

    def __getitem__(self, layer_idx):
        if layer_idx < len(self.key_cache):
            return (self.key_cache[layer_idx], self.value_cache[layer_idx])
        return (None, None)

    def to_legacy_cache(self):
        return ()

    def get_seq_length(self, layer_idx=0):
        return self._seen_tokens

    def get_max_length(self):
        return None

    def get_usable_length(self, new_seq_length, layer_idx=0):
        return self._seen_tokens

    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        self._seen_tokens += key_states.shape[-2]
        return key_states, value_states

    @property
    def seen_tokens(self):
        return self._seen_tokens


class ECCShimConfig:
    """Codec / BER / injection settings of the shim (ecc_shim.py:134-186).

    ``backend`` selects the codec implementation from kvecc.backends
    (default "hip"; unknown names raise ValueError).  ``fused`` runs the cache
    write and read as one launch each (kvecc_shim_write / kvecc_shim_read);
    False composes the per-op kernels (identical bits, kept for A/B tests).
    ``scale_rule`` picks how the INT4 row scale absmax / 7 is rounded:
    "mul_inv7" (absmax * RN(1/7), what the reference computes on GPU tensors),
    "div7" (IEEE division, the reference on CPU tensors) or None for the
    backend's device (kvecc.h KVECC_SCALE_*).
    ``golay_storage`` is the Golay cache layout: "int32" (the reference's, one
    int32 per codeword) or "packed" (3-byte codewords, token rows padded to 4
    bytes: 132 instead of 172 B per row at head_dim 128).  "packed" needs the
    fused write / read.
    ``cache_mode`` is "overwrite" (the reference's behaviour and the default:
    one cache for the whole batch, every forward writes from position 0) or
    "append": batch row b is sequence b with its own blocks, and every forward
    appends its tokens at the sequence's current length, so a patched model
    generates token by token.  "append" needs a fused codec (int4, hamming74,
    hamming84, golay) and fused=True.  ``decode_stats`` (append mode) sends
    single-token steps through the counting read instead of the paged
    attention kernels, which keep no statistics.  ``chunk_attention`` (append
    mode, opt-in) sends the forwards of more than one token -- the prefill, a
    chunk of it, the draft tokens of a verify step -- through the chunked
    causal paged attention kernel (kvecc_paged_attention_chunk) instead of the
    batched read + masked SDPA, under the decode step's conditions (hamming84
    or golay, no interpolation, decode_stats off, head_dim <= 256).  Like the
    decode step it keeps no decode statistics, which the default prefill does
    count: that is why it is off by default.  It was faster than the default
    path in every case measured (fp16, head_dim 128, 4- and 16-token chunks,
    MHA and 4 query heads per cache head: profiles/chunk_attention/); fp32 and
    bf16 models and other head_dims run the split kernels once per query row,
    which re-decode the cache for each and have not been measured.
    ``interp_attention`` (append mode, hamming84 with use_interpolation,
    opt-in) sends every forward -- single-token steps, the prefill, chunks,
    ragged spans -- through the interpolating paged attention
    (kvecc_paged_attention_interp) when decode_stats is off and head_dim <= 256:
    detected double errors are interpolated inside the kernel, no dense K / V
    is read.  It keeps no statistics either.  Each sequence's last token clamps
    at its own length, where the batched read interpolates a shorter sequence's
    last token against the zero row past it.
    ``kernel_attention`` (append mode, hamming74 or int4 only, opt-in) sends
    every forward of those two codecs through the paged attention kernels when
    decode_stats is off and head_dim <= 256: single-token steps to the decode
    entry, forwards of more than one token to the chunked causal entry, held
    spans to the ragged entry, the query read in place.  It is a flag, where
    hamming84 and golay decode steps take the kernel by default, because these
    two codecs count decode statistics on every forward today: with the flag
    on NO decode statistics are kept (``chunk_attention`` alone leaves these
    codecs on the read + SDPA path).  For hamming74, scrub_ecc_cache still
    supplies the counts; int4 has nothing to count.
    ``stats_attention`` (append mode, hamming84 with or without
    use_interpolation, opt-in) sends every forward of ``_append_attend`` --
    single-token steps, the prefill, chunks, held spans -- through the counted
    paged attention (kvecc_paged_attention_stats) when head_dim <= 256: the
    kernels count the SINGLE_CORRECTED / DOUBLE_DETECTED bytes they read into the
    shim's statistics, exactly what ``decode_stats=True`` counts through the
    read + SDPA path, and interpolate doubles inline iff use_interpolation.  It
    takes precedence over decode_stats, chunk_attention and interp_attention;
    head_dim > 256 falls back to the read + SDPA path.  One deliberate
    difference: with held spans, a sequence that has no valid
    token in the forward is not read and so not counted, where the rectangular
    read counts it.
    ``counted_attention`` (append mode, hamming84 or golay with either
    golay_storage, opt-in) is that route whatever the protected codec: for
    hamming84 it is ``stats_attention`` itself (interpolation included); for
    golay every forward of ``_append_attend`` -- every q_len, every held span --
    goes through kvecc_paged_attention_golay_stats when head_dim <= 256, which
    adds the bits corrected / uncorrectable words of the codewords it reads to
    the shim's statistics, exactly ``decode_stats=True``'s counts, with the same
    precedence, fall-back and held-span difference as ``stats_attention``.
    ``repair_attention`` (append mode, hamming84 with or without
    use_interpolation, opt-in) is ``stats_attention`` with read-repair: every
    forward of ``_append_attend`` goes through kvecc_paged_attention_repair when
    head_dim <= 256, which gives the counted call's outputs and counts and writes
    the corrected codeword back over every single-error or parity-only byte it
    reads -- the layer's resident cache comes out as scrub_ecc_cache(model,
    layers=[layer]) would leave it, on every forward, with no separate pass to
    schedule.  It takes ``stats_attention``'s place and precedence (and its
    fall-back above head_dim 256, which repairs nothing); the bytes rewritten
    accumulate in get_ecc_repaired(model).  A sequence held at count 0 is neither
    read nor repaired, and the other codecs, layers that are not being read and
    the scales still need the scrubber.
    ``attention_window`` = W > 0 (append mode, all four append codecs, opt-in)
    is sliding-window attention with ``attention_sinks`` = S sink tokens: a
    query at position p sees the keys j <= p with j > p - W or j < S.
    Positions stay absolute -- Mistral-style masking over the stored, post-RoPE
    keys; nothing in the cache is re-indexed.  Every forward
    of ``_append_attend`` goes through kvecc_paged_attention_window when
    head_dim <= 256, with or without held spans; above that the read + SDPA
    path applies the same rule in its mask.  Plain attention only: a window
    raises ValueError together with use_interpolation, decode_stats,
    interp_attention, stats_attention, counted_attention or repair_attention.
    ``evict_blocks`` (needs a window) gives blocks that no future query can see
    back to the pool before every forward, so a sequence keeps about S + W
    tokens resident however long it runs (SimpleBlockManager.evict;
    evict_ecc_cache(model) does it on request).  Eviction is host work -- it
    edits the manager's lists and uploads the released ids -- so
    ``evict_blocks`` is not for forwards captured in a HIP graph: a replay
    skips the host logic (and the host lengths the rule reads), so nothing is
    evicted; use it with eager forwards.  The block table stays
    num_blocks columns wide: a sequence can reach num_blocks * block_size
    logical tokens.
    The size condition: the interpolating, counted and repairing kernels
    (``interp_attention``, ``stats_attention``, ``counted_attention``,
    ``repair_attention``) address the caches with 32-bit buffer offsets, so beside
    head_dim <= 256 those routes need each cache, and each scale array, under
    4 GiB (SimpleBlockManager.fits_buffer_kernels, from num_blocks and the
    model's shape).  Over a larger pool they fall back exactly as above head_dim
    256: the read + SDPA path, decode_stats=True's statistics, interpolation in
    the read, nothing repaired.  The plain, windowed and ``kernel_attention``
    routes have 64-bit-addressed kernels and do not depend on the size.
    The error counts those paths do not keep are a by-product of
    scrub_ecc_cache(model), which also repairs the resident codewords in place.
    """

    SUPPORTED_CODECS = {"fp16", "fp8", "int4", "hamming74", "hamming84", "golay"}
    APPEND_CODECS = ("int4", "hamming74", "hamming84", "golay")

    def __init__(self, codec="hamming84", ber=0.0, block_size=16, num_blocks=256,
                 inject_errors=False, seed=42, use_interpolation=False, backend="hip",
                 fused=True, scale_rule=None, golay_storage="int32", cache_mode="overwrite",
                 decode_stats=False, chunk_attention=False, interp_attention=False, kernel_attention=False,
                 stats_attention=False, counted_attention=False, repair_attention=False,
                 attention_window=0, attention_sinks=0, evict_blocks=False):
        if codec not in self.SUPPORTED_CODECS:
            raise ValueError(f"Unsupported codec: '{codec}'. "
                             f"Supported codecs: {sorted(self.SUPPORTED_CODECS)}")
        self.codec = codec
        self.ber = ber
        self.block_size = block_size
        self.num_blocks = num_blocks
        self.inject_errors = inject_errors
        self.seed = seed
        self.use_interpolation = use_interpolation
        self.backend = backend
        self.fused = fused  # one-launch cache write / read (False: per-op kernels)
        self.scale_rule = scale_rule
        if golay_storage not in ("int32", "packed"):
            raise ValueError(f"golay_storage must be 'int32' or 'packed', not {golay_storage!r}")
        if golay_storage == "packed" and not fused:
            raise ValueError("golay_storage='packed' needs fused=True")
        self.golay_storage = golay_storage
        if cache_mode not in ("overwrite", "append"):
            raise ValueError(f"cache_mode must be 'overwrite' or 'append', not {cache_mode!r}")
        if cache_mode == "append" and (codec not in self.APPEND_CODECS or not fused):
            raise ValueError(f"cache_mode='append' needs fused=True and one of {self.APPEND_CODECS}, "
                             f"not codec={codec!r}, fused={fused}")
        self.cache_mode = cache_mode
        self.decode_stats = decode_stats
        if chunk_attention and cache_mode != "append":
            raise ValueError("chunk_attention=True needs cache_mode='append'")
        self.chunk_attention = bool(chunk_attention)
        if interp_attention and (cache_mode != "append" or codec != "hamming84" or not use_interpolation):
            raise ValueError("interp_attention=True needs cache_mode='append', codec='hamming84' and "
                             "use_interpolation=True")
        self.interp_attention = bool(interp_attention)
        if kernel_attention and (cache_mode != "append" or codec not in ("hamming74", "int4")):
            raise ValueError("kernel_attention=True needs cache_mode='append' and codec 'hamming74' or 'int4' "
                             f"(hamming84 and golay take the kernels by default), not codec={codec!r}, "
                             f"cache_mode={cache_mode!r}")
        self.kernel_attention = bool(kernel_attention)
        if stats_attention and (cache_mode != "append" or codec != "hamming84"):
            raise ValueError("stats_attention=True needs cache_mode='append' and codec='hamming84', "
                             f"not codec={codec!r}, cache_mode={cache_mode!r}")
        self.stats_attention = bool(stats_attention)
        if counted_attention and (cache_mode != "append" or codec not in ("hamming84", "golay")):
            raise ValueError("counted_attention=True needs cache_mode='append' and codec 'hamming84' or 'golay', "
                             f"not codec={codec!r}, cache_mode={cache_mode!r}")
        self.counted_attention = bool(counted_attention)
        if repair_attention and (cache_mode != "append" or codec != "hamming84"):
            raise ValueError("repair_attention=True needs cache_mode='append' and codec='hamming84', "
                             f"not codec={codec!r}, cache_mode={cache_mode!r}")
        self.repair_attention = bool(repair_attention)
        for name, v in (("attention_window", attention_window), ("attention_sinks", attention_sinks)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be an int >= 0, got {v!r}")
        if attention_window:
            if cache_mode != "append":
                raise ValueError("attention_window needs cache_mode='append'")
            clash = [n for n, on in (("use_interpolation", use_interpolation), ("decode_stats", decode_stats),
                                     ("interp_attention", interp_attention), ("stats_attention", stats_attention),
                                     ("counted_attention", counted_attention),
                                     ("repair_attention", repair_attention)) if on]
            if clash:
                raise ValueError(f"attention_window is plain attention only: it does not go with {', '.join(clash)}")
        if evict_blocks and not attention_window:
            raise ValueError("evict_blocks=True needs attention_window > 0: without a window every block stays visible")
        self.attention_window = int(attention_window)
        self.attention_sinks = int(attention_sinks)
        self.evict_blocks = bool(evict_blocks)


class SimpleBlockManager:
    """Paged KV storage, layout identical to ecc_shim.py:189-360.

    k_cache / v_cache: [num_blocks, num_layers, num_kv_heads, codewords_per_head]
    with codewords_per_head = block_size * head_dim (uint8 codewords, fp16,
    fp8) or block_size * ceil(head_dim/3) (int32 Golay codewords), or with
    golay_storage="packed" block_size * KVECC_GOLAY_PACKED_ROW(ceil(head_dim/3))
    uint8 (3-byte Golay codewords, not a reference layout);
    k_scales / v_scales: fp32 [num_blocks, num_layers, num_kv_heads, block_size].

    Append mode (not in the reference) adds ctx_lens, int32 [num_layers,
    max_seqs] on the device: how many tokens each layer holds of each sequence,
    with extend / advance / free; callers that never append see no change.
    """

    def __init__(self, num_blocks, block_size, num_layers, num_kv_heads, head_dim, device="cuda",
                 codec="hamming84", golay_storage="int32"):
        self.num_blocks = num_blocks
        self.block_size = block_size
        self.num_layers = num_layers
        self.num_kv_heads = num_kv_heads
        self.head_dim = head_dim
        self.device = device
        self.codec = codec
        self.needs_scales = codec not in ("fp16", "fp8")
        self.golay_packed = codec == "golay" and golay_storage == "packed"
        # the codec name the fused shim kernels take (ops.SHIM_CODECS)
        self.shim_codec = "golay_packed" if self.golay_packed else codec
        if self.golay_packed:
            self.values_per_head = block_size * golay_packed_row_bytes((head_dim + 2) // 3)
            self.cache_dtype = torch.uint8
        elif codec == "golay":
            self.values_per_head = block_size * ((head_dim + 2) // 3)
            self.cache_dtype = torch.int32
        else:
            self.values_per_head = block_size * head_dim
            self.cache_dtype = {"fp16": torch.float16, "fp8": torch.float8_e4m3fn}.get(
                codec, torch.uint8)
        self.codewords_per_head = self.values_per_head
        shape = (num_blocks, num_layers, num_kv_heads, self.codewords_per_head)
        # one allocation, V skewed off K's HBM channels (memory_layout.kv_cache_pair)
        self.k_cache, self.v_cache = kv_cache_pair(shape, self.cache_dtype, device)
        sshape = (num_blocks, num_layers, num_kv_heads, block_size)
        self.k_scales = torch.zeros(sshape, dtype=torch.float32, device=device)
        self.v_scales = torch.zeros(sshape, dtype=torch.float32, device=device)
        # whether the paged attention kernels address these caches through buffer descriptors
        # (the interpolating, counted and repairing kernels exist in that form only)
        self.buffer_addressable = self.fits_buffer_kernels(
            num_blocks, num_layers, num_kv_heads, block_size, head_dim, codec, golay_storage)
        self.free_blocks = list(range(num_blocks))
        self.seq_to_blocks = {}
        self.seq_to_len = {}
        self.max_seqs = 32
        self.max_blocks_per_seq = num_blocks
        self.block_table = torch.full((self.max_seqs, self.max_blocks_per_seq), -1,
                                      dtype=torch.int32, device=device)
        self._host_table = {}  # seq_id -> list of physical blocks (mirror, no device reads)
        # physical block ids on the device: a contiguous run of new blocks is
        # written into the table with a device-to-device copy, so allocation in
        # a steady-state forward issues no host-to-device transfer and the
        # whole patched forward can be captured in a HIP graph
        self._block_ids = torch.arange(num_blocks, dtype=torch.int32, device=device)
        # append mode: every layer's context length of every sequence, on the
        # device (the append write's start_pos, the paged attention's
        # context_lens) with a host mirror (allocation, max_context_len)
        self.ctx_lens = torch.zeros((num_layers, self.max_seqs), dtype=torch.int32, device=device)
        self._host_lens = [[0] * self.max_seqs for _ in range(num_layers)]

    @staticmethod
    def fits_buffer_kernels(num_blocks, num_layers, num_kv_heads, block_size, head_dim, codec="hamming84",
                            golay_storage="int32"):
        """True iff a cache of this shape and storage is under the 4 GiB switch of
        the paged attention entries (csrc/attention.hip, attn_setup's `fits`): one
        cache's bytes and one scale array's bytes (4 per token row) both fit 32 bits.
        Below it the kernels use 32-bit buffer offsets; at and above it only the
        plain, windowed and byte-codec entries have kernels, and the interpolating,
        counted and repairing entries return KVECC_EINVAL."""
        rows = num_blocks * num_layers * num_kv_heads * block_size
        if codec == "golay":
            g = (head_dim + 2) // 3
            row_bytes = golay_packed_row_bytes(g) if golay_storage == "packed" else 4 * g
        else:  # one byte per value (int4, hamming74, hamming84)
            row_bytes = head_dim
        return rows * row_bytes <= 0xFFFFFFFF and rows * 4 <= 0xFFFFFFFF

    # ---- append mode: per-sequence, per-layer lengths ----------------------------
    def layer_lens(self, layer, batch):
        """Host mirror of ctx_lens[layer, :batch]."""
        return self._host_lens[layer][:batch]

    def advance(self, layer, batch, num_tokens):
        """Layer `layer` of sequences [0, batch) grew by num_tokens (no host read)."""
        self.ctx_lens[layer, :batch] += num_tokens
        row = self._host_lens[layer]
        for b in range(batch):
            row[b] += num_tokens

    def advance_spans(self, layer, batch, spans, counts):
        """The per-sequence form of advance: sequence b grew by its span's count.
        The device side adds the count column of `spans` (the device [.., 3] span
        buffer, no host read), the host mirror the host `counts`."""
        self.ctx_lens[layer, :batch] += spans[:batch, 1]
        row = self._host_lens[layer]
        for b in range(batch):
            row[b] += counts[b]

    def extend(self, seq_id, new_len):
        """Blocks to cover new_len tokens of seq_id; the ones it has stay as they are."""
        if new_len > self.seq_to_len.get(seq_id, 0):
            self.allocate(seq_id, new_len)
        return self.block_table[seq_id]

    def free(self, seq_id):
        """Return seq_id's blocks, zeroed: zero codewords decode clean, so a
        re-used block adds no stale statistics."""
        blocks = [x for x in self.seq_to_blocks.pop(seq_id, []) if x >= 0]  # (evicted positions hold -1)
        self.seq_to_len.pop(seq_id, None)
        self._host_table.pop(seq_id, None)
        if blocks:
            idx = torch.tensor(blocks, dtype=torch.long, device=self.k_cache.device)
            for t in (self.k_cache, self.v_cache, self.k_scales, self.v_scales):
                t[idx] = 0
            self.free_blocks.extend(blocks)
            self.free_blocks.sort()
        self.block_table[seq_id].fill_(-1)
        self.ctx_lens[:, seq_id] = 0
        for row in self._host_lens:
            row[seq_id] = 0

    def evict(self, seq_id, window, sinks):
        """Release the blocks of seq_id that no future query can see under a
        sliding window of `window` keys with `sinks` sink tokens; returns how many.

        Lmin is the smallest length of the sequence over all layers (host mirror):
        every query still to come sits at a position >= Lmin.  Logical block lb
        is releasable iff lb * bs >= sinks (it holds no sink token) and
        (lb + 1) * bs - 1 <= Lmin - window (its last token lies before the window
        of position Lmin, hence of every later one).  A released block is zeroed
        as free() zeroes it and goes back to the sorted free list; its table
        entry becomes -1, which every kernel skips, and seq_to_blocks /
        _host_table keep a -1 at its logical position, so allocate() goes on
        counting logical blocks."""
        blocks = self.seq_to_blocks.get(seq_id)
        if not blocks or window <= 0:
            return 0
        bs = self.block_size
        lmin = min(row[seq_id] for row in self._host_lens)
        first = -(-sinks // bs)  # the first block that holds no sink token
        end = min((lmin - window + 1) // bs, len(blocks))  # exclusive: (lb + 1) * bs <= lmin - window + 1
        gone = [blocks[lb] for lb in range(first, end) if blocks[lb] >= 0]
        if not gone:  # nothing new: no device work
            return 0
        for lb in range(first, end):
            blocks[lb] = -1
        idx = torch.tensor(gone, dtype=torch.long, device=self.k_cache.device)
        for t in (self.k_cache, self.v_cache, self.k_scales, self.v_scales):
            t[idx] = 0
        self.free_blocks.extend(gone)
        self.free_blocks.sort()
        self.block_table[seq_id, first:end].fill_(-1)
        return len(gone)

    def allocate(self, seq_id, num_tokens):
        need = (num_tokens + self.block_size - 1) // self.block_size
        existing = self.seq_to_blocks.get(seq_id, [])
        new_needed = max(0, need - len(existing))  # logical blocks: evicted positions stay in the list as -1
        if new_needed > len(self.free_blocks):
            raise RuntimeError(f"Out of blocks: need {new_needed}, have {len(self.free_blocks)}")
        new = [self.free_blocks.pop(0) for _ in range(new_needed)]
        blocks = existing + new
        self.seq_to_blocks[seq_id] = blocks
        self.seq_to_len[seq_id] = num_tokens
        if new:
            dst = self.block_table[seq_id, len(existing):len(blocks)]
            if new == list(range(new[0], new[0] + len(new))):
                dst.copy_(self._block_ids[new[0]:new[0] + len(new)])
            else:
                dst.copy_(torch.tensor(new, dtype=torch.int32, device=self.block_table.device))
        self._host_table[seq_id] = blocks
        return self.block_table[seq_id], num_tokens

    def get_block_table(self, seq_id):
        return self.block_table[seq_id]

    def get_context_len(self, seq_id):
        return self.seq_to_len.get(seq_id, 0)

    def reset(self):
        # every block back in ascending order.  The reference appends the
        # returned blocks to the free list (ecc_shim.py:349-353), so each reset
        # rotates the physical ids the next forward gets; nothing observable
        # depends on them (the caches are zeroed here), but torch.compile
        # specialises a traced forward's allocation on the free list, and a
        # rotating list recompiled the patched model on every forward
        for blocks in self.seq_to_blocks.values():
            self.free_blocks.extend(x for x in blocks if x >= 0)  # (evicted positions hold -1)
        self.free_blocks.sort()
        self.seq_to_blocks.clear()
        self.seq_to_len.clear()
        self._host_table.clear()
        self.block_table.fill_(-1)
        self.ctx_lens.zero_()
        for row in self._host_lens:
            row[:] = [0] * self.max_seqs
        self.k_cache.zero_()
        self.v_cache.zero_()
        self.k_scales.zero_()
        self.v_scales.zero_()

    # ---- vectorised slot addressing -------------------------------------------
    def slots(self, seq_id, positions: int):
        """(physical block, slot) index tensors of token positions [0, positions)."""
        blocks = self._host_table.get(seq_id, [])
        pos = torch.arange(positions, device=self.k_cache.device)
        tab = torch.tensor(blocks or [0], dtype=torch.long, device=self.k_cache.device)
        return tab[pos // self.block_size], pos % self.block_size

    def view5(self, cache):
        """[blocks, layers, heads, block_size, per_token] view of a cache tensor."""
        return cache.view(self.num_blocks, self.num_layers, self.num_kv_heads, self.block_size, -1)


# age_ecc_cache draws V's flips with seed + V_SEED_OFFSET: consecutive seeds (one
# per round of an experiment) then never give K of one round V's draw of another
V_SEED_OFFSET = 1_000_003

_N_BITS = {"hamming74": 7, "hamming84": 8, "golay": 24, "int4": 4, "fp8": 8}


class ECCBackend:
    """Quantize/encode/inject on write, decode/correct/dequantize on attend.

    Same observable behaviour as ecc_shim.py:363-1164: per-row injection seeds
    (K: seed + count, V: seed + count + 1, count += 1 per (batch, pos, head)
    row), last-batch-wins cache writes, statistics semantics per codec.
    """

    # codecs whose write / read run as one fused launch each (shim.hip)
    FUSED_CODECS = ("int4", "hamming74", "hamming84", "golay")

    def __init__(self, manager, config, num_heads, fused=None):
        self.manager = manager
        self.config = config
        self.codec_backend = get_codec_backend(getattr(config, "backend", "hip"))
        # fused=False composes the per-op kernels instead (same bits; A/B tests)
        self.fused = getattr(config, "fused", True) if fused is None else fused
        self.num_heads = num_heads
        self.num_kv_heads = manager.num_kv_heads
        self.head_dim = manager.head_dim
        if manager.golay_packed and not self._fused_ok():
            raise ValueError("packed Golay storage needs the fused shim write / read "
                             "(fused=True, a backend with shim_write, head_dim <= 512)")
        self.append = getattr(config, "cache_mode", "overwrite") == "append"
        if self.append and not (self._fused_ok() and hasattr(self.codec_backend, "shim_append_tensors")):
            raise ValueError("cache_mode='append' needs the fused shim kernels (fused=True, a backend with "
                             "shim_append_tensors, head_dim <= 512 and a multiple of 4 for the byte codecs)")
        self.num_kv_groups = num_heads // self.num_kv_heads
        self._injection_count = 0
        self._total_values = 0
        self._stats = self.codec_backend.new_stats(manager.k_cache.device)  # backend counters
        if getattr(config, "repair_attention", False):
            # the repairing attention adds the bytes it rewrites to word 2, which no other
            # writer of this buffer touches: a buffer with that word on every backend
            if not hasattr(self.codec_backend, "paged_attention_repair_into"):
                raise ValueError("repair_attention=True needs a backend with paged_attention_repair_into")
            self._stats = self.codec_backend.new_scrub_stats(manager.k_cache.device)
        # cumulative counters of scrub() alone (corrected, detected, rewritten,
        # scanned), allocated by the first scrub; get_ecc_stats never reads them
        self._scrub_stats = None
        self._scrub_len = {}  # overwrite mode: context length -> its one-element device tensor
        # ragged batches (set_query_spans): host (counts, firsts) and the
        # persistent device buffer [max_seqs, 3] the kernels read
        self._spans = None
        self._span_buf = None

    # counters read lazily (one sync) -------------------------------------------
    @property
    def _errors_corrected(self):
        return self.codec_backend.read_stats(self._stats, 2)[0]

    @property
    def _errors_detected(self):
        return self.codec_backend.read_stats(self._stats, 2)[1]

    def reset_stats(self):
        self._injection_count = 0
        self._total_values = 0
        self._stats.zero_()
        if self._scrub_stats is not None:
            self._scrub_stats.zero_()

    # ---- cache scrub (no reference counterpart) -----------------------------------
    SCRUB_CODECS = ("hamming74", "hamming84", "golay")

    def _layer_runs(self, layers):
        """Runs (first, count) of consecutive layers covering `layers` (None: all)."""
        n = self.manager.num_layers
        if layers is None:
            return [(0, n)]
        ls = sorted({int(x) for x in ([layers] if isinstance(layers, int) else layers)})
        if any(not 0 <= x < n for x in ls):
            raise ValueError(f"layers {ls} outside the cache's {n} layers")
        runs = []
        for x in ls:
            if runs and runs[-1][0] + runs[-1][1] == x:
                runs[-1][1] += 1
            else:
                runs.append([x, 1])
        return [tuple(r) for r in runs]

    def scrub(self, layers=None):
        """Correct and re-encode the resident codewords of `layers` (None: every
        layer) in place, all live sequences in one launch (one per run of
        consecutive layers): a correctable word that differs from
        encode(decoded data) is rewritten, so errors stop piling up in a cache
        that stays resident for a whole generation.  Append mode scrubs every
        sequence up to its own per-layer length, overwrite mode sequence 0.
        Counts add into a scrub-only buffer (scrub_totals()); the decode
        statistics of get_ecc_stats are not touched.  Nothing is read back, so
        the call can be captured in a HIP graph between forwards."""
        cfg, mgr = self.config, self.manager
        if cfg.codec not in self.SCRUB_CODECS:
            raise ValueError(f"codec {cfg.codec!r} has no ECC: nothing to scrub (one of {self.SCRUB_CODECS})")
        be = self.codec_backend
        if not hasattr(be, "cache_scrub_tensors"):
            raise ValueError("this backend has no cache scrub (cache_scrub_tensors)")
        if self._scrub_stats is None:
            self._scrub_stats = be.new_scrub_stats(mgr.k_cache.device)
        fn = self._scrub_op if self._traced() else be.cache_scrub_tensors
        for first, count in self._layer_runs(layers):
            if self.append:
                batch = max(mgr.seq_to_blocks, default=-1) + 1  # sequences are 0 .. batch-1
                if batch == 0:
                    continue
                mcl = max(max(mgr.layer_lens(l, batch)) for l in range(first, first + count))
                if mcl == 0:
                    continue
                fn(mgr.k_cache, mgr.v_cache, mgr.block_table[:batch], mgr.ctx_lens[first:first + count],
                   self.head_dim, mgr.block_size, mgr.num_layers, mgr.shim_codec, first, count, mcl,
                   self._scrub_stats)
            else:
                n = mgr.get_context_len(0)
                if n == 0:
                    continue
                lens = self._scrub_len.get(n)
                if lens is None:  # a device fill, no host-to-device copy
                    lens = self._scrub_len[n] = torch.full((1,), n, dtype=torch.int32, device=mgr.k_cache.device)
                fn(mgr.k_cache, mgr.v_cache, mgr.block_table[0:1], lens, self.head_dim, mgr.block_size,
                   mgr.num_layers, mgr.shim_codec, first, count, n, self._scrub_stats)

    @staticmethod
    def _scrub_op(*args):
        torch.ops.kvecc.cache_scrub(*args)

    def scrub_totals(self):
        """Device int64 [4] of the cumulative scrub counters (corrected, detected,
        rewritten, scanned) since the last reset; no host sync."""
        if self._scrub_stats is None:
            return torch.zeros(4, dtype=torch.int64, device=self.manager.k_cache.device)
        return self.codec_backend.stats_totals(self._scrub_stats, 4)

    def age(self, ber, seed):
        """Residency-error model: in-place Bernoulli flips over the WHOLE K and V
        cache tensors (V with seed + V_SEED_OFFSET); see age_ecc_cache."""
        cfg, mgr = self.config, self.manager
        if cfg.codec not in self.SCRUB_CODECS:
            raise ValueError(f"codec {cfg.codec!r} has no ECC cache to age (one of {self.SCRUB_CODECS})")
        if not ber > 0:
            return
        n_bits = 8 if mgr.golay_packed else _N_BITS[cfg.codec]
        for i, cache in enumerate((mgr.k_cache, mgr.v_cache)):
            torch.ops.kvecc.inject_bit_errors_(cache, float(ber), n_bits, int(seed) + i * V_SEED_OFFSET)

    def _inject_rows(self, enc, rows, row_len, seed_base):
        """Per-row injection of the reference's write loop, in place."""
        flat = enc.view(-1) if enc.dtype != torch.float8_e4m3fn else enc.view(torch.uint8).view(-1)
        self.codec_backend.inject_rows_into(flat, flat, rows, row_len, self.config.ber,
                             _N_BITS[self.config.codec], seed_base)

    def write(self, k, v, layer_idx, seq_id=0):
        """Store K, V [batch, seq, kv_heads*head_dim] (or a [batch, seq, kv_heads,
        head_dim] view, which the fused path reads in place) for layer `layer_idx`."""
        if self.append:
            return self._append_write(k, v, layer_idx)
        cfg, mgr = self.config, self.manager
        batch, seq_len = k.shape[0], k.shape[1]
        d, hk = self.head_dim, self.num_kv_heads
        self._total_values += 2 * batch * seq_len * hk * d
        if mgr.get_context_len(seq_id) < seq_len:
            mgr.allocate(seq_id, seq_len)
        rows = batch * seq_len * hk
        inject = cfg.inject_errors and cfg.ber > 0
        seed0 = cfg.seed + self._injection_count
        if self._fused_ok(k) and k.dtype == v.dtype:
            if self._traced():  # torch.compile: the dispatcher operator (no graph break)
                torch.ops.kvecc.shim_write(k, v, mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales,
                                           mgr.block_table[seq_id], mgr.num_layers, mgr.block_size,
                                           mgr.num_kv_heads, mgr.head_dim, layer_idx, mgr.shim_codec,
                                           _N_BITS[cfg.codec], inject, cfg.ber, seed0, cfg.scale_rule)
            else:
                self.codec_backend.shim_write(k, v, mgr, layer_idx, mgr.shim_codec, _N_BITS[cfg.codec],
                                              inject, cfg.ber, seed0, seq_id, cfg.scale_rule)
            if inject:
                self._injection_count += rows
            return
        if mgr.golay_packed:
            raise TypeError(f"packed Golay storage: K/V dtype {k.dtype}/{v.dtype} has no fused write")
        blk, slot = mgr.slots(seq_id, seq_len)
        kr = k.reshape(batch, seq_len, hk, d)
        vr = v.reshape(batch, seq_len, hk, d)
        codec = cfg.codec
        ops = self.codec_backend
        for which, x, cache, scales in ((0, kr, mgr.k_cache, mgr.k_scales),
                                        (1, vr, mgr.v_cache, mgr.v_scales)):
            if codec == "fp16":
                enc = x.to(torch.float16)
            elif codec == "fp8":
                enc = x.to(torch.float8_e4m3fn).contiguous()
                if inject:
                    self._inject_rows(enc, rows, d, seed0 + which)
            else:
                q, sc = ops.quantize_rows(x, cfg.scale_rule)  # the shim's torch rounding
                if codec == "golay":
                    enc = ops.golay_encode_rows(q)
                    row_len = enc.shape[-1]
                elif codec == "hamming74":
                    enc = ops.hamming74_encode(q)
                    row_len = d
                elif codec == "hamming84":
                    enc = ops.hamming84_encode(q)
                    row_len = d
                else:  # int4: raw nibbles
                    enc = q
                    row_len = d
                if inject:
                    self._inject_rows(enc, rows, row_len, seed0 + which)
                # last batch wins (every batch writes the same seq_id slots)
                mgr.view5(scales)[blk, layer_idx, :, slot, 0] = sc[-1]
            mgr.view5(cache)[blk, layer_idx, :, slot, :] = enc[-1].to(cache.dtype)
        if inject:
            self._injection_count += rows

    # ---- append mode (no reference counterpart) -----------------------------------
    def check_append_batch(self, batch):
        if batch > self.manager.max_seqs:
            raise ValueError(f"append mode holds {self.manager.max_seqs} sequences, got a batch of {batch}")

    def set_query_spans(self, counts, firsts=None):
        """Hold per-sequence query spans for every following append-mode forward
        (None clears them): sequence b's valid tokens are [firsts[b], firsts[b] +
        counts[b]) of its row.  The spans go to the device once, here; a forward
        reads the buffer and copies nothing from the host."""
        if counts is None:
            self._spans = None
            return
        if not self.append:
            raise ValueError("query spans need cache_mode='append'")
        if not hasattr(self.codec_backend, "shim_append_ragged_tensors"):
            raise ValueError("this backend has no ragged append (shim_append_ragged_tensors)")
        counts = [int(c) for c in counts]
        firsts = [0] * len(counts) if firsts is None else [int(f) for f in firsts]
        self.check_append_batch(len(counts))
        spans = self.codec_backend.query_spans(counts, firsts)  # ValueError: a negative entry, lengths
        if self._span_buf is None:
            self._span_buf = torch.zeros((self.manager.max_seqs, 3), dtype=torch.int32,
                                         device=self.manager.k_cache.device)
        self._span_buf[:len(counts)].copy_(spans)
        self._spans = (counts, firsts)

    def _check_spans(self, batch, q_max):
        counts, firsts = self._spans
        if len(counts) != batch:
            raise ValueError(f"query spans hold {len(counts)} sequences, the forward has a batch of {batch}")
        for b, (f, c) in enumerate(zip(firsts, counts)):
            if f + c > q_max:
                raise ValueError(f"query span {b}: first {f} + count {c} > the forward's {q_max} tokens")

    def _append_write(self, k, v, layer_idx):
        """Batch row b is sequence b: its q_len tokens go behind the layer's
        current length of that sequence, every sequence in one launch.  The
        start positions are the manager's device lengths; nothing is read back.
        With query spans held, only each row's valid tokens are appended."""
        cfg, mgr = self.config, self.manager
        batch, q_len = k.shape[0], k.shape[1]
        self.check_append_batch(batch)
        if k.dtype != v.dtype or k.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"append mode: K/V dtype {k.dtype}/{v.dtype} has no fused write")
        d, hk = self.head_dim, self.num_kv_heads
        if self._spans is not None:
            self._check_spans(batch, q_len)  # before anything is written or released
        if getattr(cfg, "evict_blocks", False) and layer_idx == 0:
            # before the forward's first write (and after every check that can refuse the forward),
            # when every layer holds the same lengths: the blocks no query from here on can see go
            # back to the pool this forward allocates from.  Host work: not for a captured forward.
            self.evict()
        if self._spans is not None:
            counts = self._spans[0]
            total = sum(counts)
            self._total_values += 2 * total * hk * d
            for b, n in enumerate(mgr.layer_lens(layer_idx, batch)):
                mgr.extend(b, n + counts[b])  # count 0: nothing allocated
            inject = cfg.inject_errors and cfg.ber > 0
            seed0 = cfg.seed + self._injection_count
            spans = self._span_buf[:batch]
            if self._traced():
                torch.ops.kvecc.shim_append_ragged(
                    k, v, mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales, mgr.block_table[:batch],
                    mgr.ctx_lens[layer_idx, :batch], spans, mgr.num_layers, mgr.block_size, hk, d, layer_idx,
                    mgr.shim_codec, _N_BITS[cfg.codec], inject, cfg.ber, seed0, cfg.scale_rule)
            else:
                self.codec_backend.shim_append_ragged_tensors(
                    k, v, mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales, mgr.block_table[:batch],
                    mgr.ctx_lens[layer_idx, :batch], mgr.num_layers, mgr.block_size, hk, d, layer_idx,
                    mgr.shim_codec, _N_BITS[cfg.codec], inject, cfg.ber, seed0, spans, cfg.scale_rule)
            mgr.advance_spans(layer_idx, batch, self._span_buf, counts)
            if inject:
                self._injection_count += total * hk  # dense seeds: rows written
            return
        self._total_values += 2 * batch * q_len * hk * d
        for b, n in enumerate(mgr.layer_lens(layer_idx, batch)):
            mgr.extend(b, n + q_len)
        inject = cfg.inject_errors and cfg.ber > 0
        seed0 = cfg.seed + self._injection_count
        # the dispatcher operator while torch.compile traces, the C ABI otherwise
        fn = torch.ops.kvecc.shim_append if self._traced() else self.codec_backend.shim_append_tensors
        fn(k, v, mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales, mgr.block_table[:batch],
           mgr.ctx_lens[layer_idx, :batch], mgr.num_layers, mgr.block_size, hk, d, layer_idx, mgr.shim_codec,
           _N_BITS[cfg.codec], inject, cfg.ber, seed0, cfg.scale_rule)
        mgr.advance(layer_idx, batch, q_len)
        if inject:
            self._injection_count += batch * q_len * hk

    def evict(self):
        """Release every live sequence's blocks that lie behind its sliding window
        and hold no sink token (SimpleBlockManager.evict: the rule, from the host
        lengths of all layers); returns the number of blocks released."""
        cfg = self.config
        window, sinks = getattr(cfg, "attention_window", 0), getattr(cfg, "attention_sinks", 0)
        if not window:
            raise ValueError("eviction needs ECCShimConfig(attention_window > 0): without a window every block "
                             "stays visible")
        return sum(self.manager.evict(seq, window, sinks) for seq in list(self.manager.seq_to_blocks))

    def _append_attend(self, q, layer_idx):
        """Attention of q [batch, heads, q_len, head_dim], row b over sequence
        b's own cache; the layer's write has already advanced the lengths."""
        cfg, mgr = self.config, self.manager
        b, _, q_len, d = q.shape
        lens = mgr.layer_lens(layer_idx, b)
        ctx = max(lens)
        if ctx == 0:
            return torch.zeros_like(q)
        table, dev_lens = mgr.block_table[:b], mgr.ctx_lens[layer_idx, :b]
        interp = cfg.use_interpolation and cfg.codec == "hamming84"
        # hamming74 / int4 take the kernels only under kernel_attention (their codec is checked there)
        kernel_codec = cfg.codec in ("hamming84", "golay") or cfg.kernel_attention
        window, sinks = getattr(cfg, "attention_window", 0), getattr(cfg, "attention_sinks", 0)
        # The interpolating, counted and repairing entries have buffer-addressed kernels only
        # (caches under 4 GiB: SimpleBlockManager.fits_buffer_kernels).  On a larger cache those
        # routes fall back as they do above head_dim 256: a counting route to the read + SDPA
        # path, which counts what decode_stats=True counts (and repairs nothing), the
        # interpolating one to the read + SDPA path, which interpolates in the read.
        sized = d <= 256 and getattr(mgr, "buffer_addressable", True)  # (a manager of the caller's own: as before)
        counting = cfg.decode_stats or cfg.stats_attention or cfg.counted_attention or cfg.repair_attention
        if window and d <= 256:
            # every q_len and every append codec on the windowed kernels: q read in place as
            # [batch, q_len, heads, d]; row at p sees keys j <= p with j > p - window or j < sinks
            sp = None
            if self._spans is not None:
                self._check_spans(b, q_len)
                sp = self._span_buf[:b]
            qt = q.transpose(1, 2)
            if self._traced():
                out = torch.ops.kvecc.paged_attention_window(
                    qt, mgr.k_cache, mgr.v_cache, table, dev_lens, sp, mgr.k_scales, mgr.v_scales, layer_idx,
                    mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, window, sinks, ctx)
                return out.transpose(1, 2)
            if not hasattr(self.codec_backend, "paged_attention_window_into"):
                raise ValueError("attention_window needs a backend with paged_attention_window_into")
            out = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
            self.codec_backend.paged_attention_window_into(
                qt, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, window, sinks, max_context_len=ctx, q_spans=sp)
            return out.transpose(1, 2)
        if cfg.counted_attention and cfg.codec == "golay" and sized:
            # every q_len on the Golay counted kernels (int32 or packed rows): the bits
            # corrected / uncorrectable words of the codewords read added to the shim's buffer
            sp = None
            if self._spans is not None:
                self._check_spans(b, q_len)
                sp = self._span_buf[:b]
            qt = q.transpose(1, 2)
            if self._traced():
                out = torch.ops.kvecc.paged_attention_golay_stats(
                    qt, mgr.k_cache, mgr.v_cache, table, dev_lens, sp, mgr.k_scales, mgr.v_scales, self._stats,
                    layer_idx, mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, ctx)
                return out.transpose(1, 2)
            out = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
            self.codec_backend.paged_attention_counted_into(
                qt, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, self._stats, max_context_len=ctx, q_spans=sp)
            return out.transpose(1, 2)
        if cfg.repair_attention and sized:
            # the counted route below on the repairing kernels: the same outputs and counts, and
            # the correctable bytes read are rewritten in mgr.k_cache / mgr.v_cache in place
            sp = None
            if self._spans is not None:
                self._check_spans(b, q_len)
                sp = self._span_buf[:b]
            qt = q.transpose(1, 2)
            if self._traced():
                out = torch.ops.kvecc.paged_attention_repair(
                    qt, mgr.k_cache, mgr.v_cache, table, dev_lens, sp, mgr.k_scales, mgr.v_scales, self._stats,
                    layer_idx, mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, interp, ctx)
                return out.transpose(1, 2)
            out = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
            self.codec_backend.paged_attention_repair_into(
                qt, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, self._stats, max_context_len=ctx, q_spans=sp,
                interp=interp)
            return out.transpose(1, 2)
        if (cfg.stats_attention or cfg.counted_attention) and sized:  # (counted_attention: hamming84 here)
            # every q_len on the counted kernels: q read in place as [batch, q_len,
            # heads, d], the decode statistics of the bytes read added to the shim's
            # buffer, doubles interpolated inline iff use_interpolation
            sp = None
            if self._spans is not None:
                self._check_spans(b, q_len)
                sp = self._span_buf[:b]
            qt = q.transpose(1, 2)
            if self._traced():
                out = torch.ops.kvecc.paged_attention_stats(
                    qt, mgr.k_cache, mgr.v_cache, table, dev_lens, sp, mgr.k_scales, mgr.v_scales, self._stats,
                    layer_idx, mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, interp, ctx)
                return out.transpose(1, 2)
            out = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
            self.codec_backend.paged_attention_chunk_into(
                qt, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, max_context_len=ctx, q_spans=sp,
                interp=interp, stats=self._stats)
            return out.transpose(1, 2)
        if q_len == 1 and kernel_codec and not interp and not counting and d <= 256:
            # decode step: paged attention with inline decode over the ragged
            # tables; no statistics, as on the reference's seq_len == 1 path
            q1 = q[:, :, 0, :].contiguous()
            if self._traced():
                out = torch.ops.kvecc.paged_attention(q1, mgr.k_cache, mgr.v_cache, table, dev_lens,
                                                      mgr.k_scales, mgr.v_scales, layer_idx, mgr.block_size,
                                                      1.0 / math.sqrt(d), mgr.shim_codec, ctx)
                return out.unsqueeze(2)
            out = torch.empty_like(q1)
            self.codec_backend.paged_attention_into(
                q1, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, max_context_len=ctx)
            return out.unsqueeze(2)
        spans = None
        if self._spans is not None:
            self._check_spans(b, q_len)
            spans = self._span_buf[:b]
        if interp and cfg.interp_attention and not counting and sized:
            # every q_len on the interpolating kernel: q read in place as [batch,
            # q_len, heads, d], doubles interpolated inline, no dense K / V, no statistics
            qt = q.transpose(1, 2)
            if self._traced():
                out = torch.ops.kvecc.paged_attention_interp(
                    qt, mgr.k_cache, mgr.v_cache, table, dev_lens, spans, mgr.k_scales, mgr.v_scales,
                    layer_idx, mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, ctx)
                return out.transpose(1, 2)
            out = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
            self.codec_backend.paged_attention_chunk_into(
                qt, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, max_context_len=ctx, q_spans=spans,
                interp=True)
            return out.transpose(1, 2)
        chunk_kernel = cfg.kernel_attention or (cfg.chunk_attention and cfg.codec in ("hamming84", "golay"))
        if q_len > 1 and chunk_kernel and not interp and not counting and d <= 256:
            # prefill / chunk / verify step on the chunked causal kernel: q read
            # in place as [batch, q_len, heads, d], no dense K / V, no statistics
            qt = q.transpose(1, 2)
            if spans is not None:  # ragged: padding rows come out as the kernel's empty value
                if self._traced():
                    out = torch.ops.kvecc.paged_attention_chunk_ragged(
                        qt, mgr.k_cache, mgr.v_cache, table, dev_lens, spans, mgr.k_scales, mgr.v_scales,
                        layer_idx, mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, ctx)
                    return out.transpose(1, 2)
                out = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
                self.codec_backend.paged_attention_chunk_into(
                    qt, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                    mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, max_context_len=ctx, q_spans=spans)
                return out.transpose(1, 2)
            if self._traced():
                out = torch.ops.kvecc.paged_attention_chunk(qt, mgr.k_cache, mgr.v_cache, table, dev_lens,
                                                            mgr.k_scales, mgr.v_scales, layer_idx,
                                                            mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec,
                                                            ctx)
                return out.transpose(1, 2)
            out = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
            self.codec_backend.paged_attention_chunk_into(
                qt, mgr.k_cache, mgr.v_cache, table, dev_lens, mgr.k_scales, mgr.v_scales, out, layer_idx,
                mgr.block_size, 1.0 / math.sqrt(d), mgr.shim_codec, max_context_len=ctx)
            return out.transpose(1, 2)
        # prefill, chunks, hamming74 / int4, interpolation, decode_stats: one
        # batched read at the longest length, then masked SDPA.  The read
        # decodes ctx rows of every sequence: a shorter sequence's rows past
        # its length are unwritten (zero codewords in a zeroed block, or no
        # block at all), decode clean and add nothing to the statistics; the
        # mask keeps them out of the attention.
        k_t, v_t = self.codec_backend.shim_read_batch(
            mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales, table, ctx, d, layer_idx, mgr.shim_codec,
            q.dtype, stats=self._stats, interp=interp)
        if self.num_kv_groups > 1:
            k_t = k_t.repeat_interleave(self.num_kv_groups, dim=1)
            v_t = v_t.repeat_interleave(self.num_kv_groups, dim=1)
        # query t of sequence b sits at position start_b + t and sees keys j <= start_b + t
        tq = torch.arange(q_len, device=q.device).view(1, q_len, 1)
        keys = torch.arange(ctx, device=q.device).view(1, 1, ctx)
        if spans is not None:
            # valid token t of sequence b sits at ctx_b - count_b + (t - first_b); a
            # padding row sees key 0 alone, so that it comes out finite
            first, count = spans[:, 0].view(b, 1, 1), spans[:, 1].view(b, 1, 1)
            valid = (tq >= first) & (tq < first + count)
            qpos = (dev_lens.view(b, 1, 1) - count) + (tq - first)
            seen = keys <= qpos
            if window:  # (head_dim > 256) the windowed rule of the kernels, in the mask
                seen = seen & ((keys > qpos - window) | (keys < sinks))
            mask = torch.where(valid, seen, keys == 0)
            return F.scaled_dot_product_attention(q, k_t, v_t, attn_mask=mask.unsqueeze(1))
        qpos = (dev_lens - q_len).view(b, 1, 1) + tq
        mask = keys <= qpos
        if window:  # (head_dim > 256) the windowed rule of the kernels, in the mask
            mask = mask & ((keys > qpos - window) | (keys < sinks))
        return F.scaled_dot_product_attention(q, k_t, v_t, attn_mask=mask.unsqueeze(1))

    def _traced(self):
        """True while torch.compile traces this backend and it is one whose
        kernels are registered as torch.ops.kvecc operators (hip, cpu): calls
        then go through the dispatcher, eager calls straight to the C ABI."""
        return torch.compiler.is_compiling() and self.codec_backend.__name__ in ("kvecc.ops", "kvecc.cpu_ops")

    def _fused_ok(self, x=None):
        if not self.fused or self.config.codec not in self.FUSED_CODECS:
            return False
        if not hasattr(self.codec_backend, "shim_write"):
            return False
        d = self.head_dim
        if self.config.codec != "golay" and d % 4:
            return False
        if d > 512:
            return False
        return x is None or x.dtype in (torch.float32, torch.float16, torch.bfloat16)

    def _gather(self, cache, blk, slot, layer_idx):
        return self.manager.view5(cache)[blk, layer_idx, :, slot, :]  # [ctx, heads, per_token]

    def _decode(self, enc, stats):
        """Codewords [ctx, heads, *] -> INT4 [ctx, heads, head_dim] (stats += ...)."""
        codec, d = self.config.codec, self.head_dim
        ops = self.codec_backend
        if codec == "golay":
            return ops.golay_decode_rows(enc, d, stats=stats)
        flat = enc.reshape(-1)
        out = torch.empty_like(flat)
        if codec == "hamming74":
            ops.hamming74_decode_into(flat, out, None, stats)
            return out.view(enc.shape)
        if codec == "hamming84":
            if self.config.use_interpolation:
                et = torch.empty_like(flat)
                ops.hamming84_decode_into(flat, out, et, stats)
                ctx = enc.shape[0]
                res = torch.empty_like(flat)
                # temporal neighbours along the context axis (ecc_shim.py:1048-1059)
                ops.interpolate_into(out, et, res, 1, ctx, flat.numel() // max(ctx, 1))
                return res.view(enc.shape)
            ops.hamming84_decode_into(flat, out, None, stats)
            return out.view(enc.shape)
        return enc  # int4: raw nibbles

    def attend(self, q, layer_idx, seq_id=0):
        """Attention of q [batch, heads, seq, head_dim] over the decoded cache."""
        if self.append:
            return self._append_attend(q, layer_idx)
        cfg, mgr = self.config, self.manager
        ctx = mgr.get_context_len(seq_id)
        if ctx == 0:
            return torch.zeros_like(q)
        q_len = q.shape[2]
        fast = cfg.codec == "hamming84" and not cfg.use_interpolation and q_len == 1
        if self._fused_ok() and fast:
            return self._paged_decode_attention(q, layer_idx, seq_id, ctx)
        if self._fused_ok():
            # the reference's seq_len==1 Triton path (ecc_shim.py:791-800) keeps no statistics
            interp = cfg.use_interpolation and cfg.codec == "hamming84"
            out_dtype, stats = (torch.float32, None) if fast else (q.dtype, self._stats)
            if self._traced():
                k_t, v_t = torch.ops.kvecc.shim_read(
                    mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales, mgr.block_table[seq_id], ctx,
                    mgr.num_kv_heads, mgr.head_dim, mgr.num_layers, mgr.block_size, layer_idx, mgr.shim_codec,
                    interp, out_dtype, stats)
            else:
                k_t, v_t = self.codec_backend.shim_read(mgr, layer_idx, ctx, mgr.shim_codec, interp,
                                                        out_dtype, stats, seq_id)
            if fast:
                return self._decode_step_attention(q, k_t, v_t)
            return self._run_attention_hd(q, k_t, v_t)
        blk, slot = mgr.slots(seq_id, ctx)
        k_enc = self._gather(mgr.k_cache, blk, slot, layer_idx)
        v_enc = self._gather(mgr.v_cache, blk, slot, layer_idx)
        if cfg.codec == "fp16":
            return self._run_attention(q, k_enc, v_enc)
        if cfg.codec == "fp8":
            return self._run_attention(q, k_enc.to(torch.float16), v_enc.to(torch.float16))
        # the reference's seq_len==1 Triton path (ecc_shim.py:791-800) keeps no statistics
        stats = None if fast else self._stats
        k_dec = self._decode(k_enc, stats)
        v_dec = self._decode(v_enc, stats)
        k_sc = mgr.view5(mgr.k_scales)[blk, layer_idx, :, slot, 0]
        v_sc = mgr.view5(mgr.v_scales)[blk, layer_idx, :, slot, 0]
        k_f = (k_dec.float() - 8.0) * k_sc.unsqueeze(-1)
        v_f = (v_dec.float() - 8.0) * v_sc.unsqueeze(-1)
        if fast:
            return self._decode_step_attention(q, k_f.transpose(0, 1), v_f.transpose(0, 1))
        return self._run_attention(q, k_f, v_f)

    def _paged_decode_attention(self, q, layer_idx, seq_id, ctx):
        """seq_len==1 Hamming(8,4) path: paged attention with inline decode
        (attention_ecc.py:620-780 via ecc_shim.py:1091-1136), no statistics.
        Every batch row attends over the same seq_id context (the reference
        passes one block-table row, ecc_shim.py:1117-1129)."""
        mgr = self.manager
        b, h, _, d = q.shape
        q1 = q[:, :, 0, :].contiguous()
        table = mgr.block_table[seq_id].unsqueeze(0).expand(b, -1).contiguous()
        lens = torch.full((b,), ctx, dtype=torch.int32, device=q.device)
        if self._traced():
            out = torch.ops.kvecc.paged_attention(q1, mgr.k_cache, mgr.v_cache, table, lens, mgr.k_scales,
                                                  mgr.v_scales, layer_idx, mgr.block_size, 1.0 / math.sqrt(d),
                                                  "hamming84", ctx)
            return out.unsqueeze(2)
        out = torch.empty_like(q1)
        self.codec_backend.paged_attention_into(
            q1, mgr.k_cache, mgr.v_cache, table, lens, mgr.k_scales, mgr.v_scales, out,
            layer_idx, mgr.block_size, 1.0 / math.sqrt(d), "hamming84", max_context_len=ctx)
        return out.unsqueeze(2)

    def _decode_step_attention(self, q, k_f, v_f):
        """seq_len==1 path of paged_attention_ecc (attention_ecc.py:264-427): fp32
        softmax over the context, output in q's dtype.  K/V are head-major
        [Hkv, ctx, D]; query head h reads cache head h // groups (the reference
        indexes cache head h directly, which only agrees without GQA)."""
        if self.num_kv_groups > 1:
            k_f = k_f.repeat_interleave(self.num_kv_groups, dim=0)
            v_f = v_f.repeat_interleave(self.num_kv_groups, dim=0)
        scale = 1.0 / math.sqrt(self.head_dim)
        qf = q[:, :, 0, :].float()                                # [B, H, D]
        scores = torch.einsum("bhd,htd->bht", qf, k_f) * scale     # [B, H, ctx]
        w = torch.softmax(scores, dim=-1)
        out = torch.einsum("bht,htd->bhd", w, v_f)
        return out.to(q.dtype).unsqueeze(2)

    def _run_attention_hd(self, q, k, v):
        """_run_attention on head-major K/V [Hkv, ctx, D] already in q's dtype."""
        if self.num_kv_groups > 1:
            k = k.repeat_interleave(self.num_kv_groups, dim=0)
            v = v.repeat_interleave(self.num_kv_groups, dim=0)
        return F.scaled_dot_product_attention(q, k.unsqueeze(0), v.unsqueeze(0),
                                              is_causal=q.shape[2] > 1)

    def _run_attention(self, q, k_float, v_float, device=None):
        """GQA expand + SDPA, causal for prefill (ecc_shim.py:1138-1164)."""
        if self.num_kv_groups > 1:
            k_float = k_float.repeat_interleave(self.num_kv_groups, dim=1)
            v_float = v_float.repeat_interleave(self.num_kv_groups, dim=1)
        k = k_float.permute(1, 0, 2).unsqueeze(0).to(q.dtype)
        v = v_float.permute(1, 0, 2).unsqueeze(0).to(q.dtype)
        return F.scaled_dot_product_attention(q, k, v, is_causal=q.shape[2] > 1)


class ECCPagedAttentionShim(nn.Module):
    """Replacement attention module (ecc_shim.py:1167-1392)."""

    def __init__(self, original_attn, layer_idx, backend, rotary_emb, model_type="llama"):
        super().__init__()
        self.model_type = model_type
        if model_type == "gpt2":
            for name in ("c_attn", "c_proj"):
                if not hasattr(original_attn, name):
                    avail = [a for a in dir(original_attn) if not a.startswith("_")]
                    raise ValueError(f"GPT-2 attention module missing '{name}'. Available: {avail}")
                setattr(self, name, getattr(original_attn, name))
            if hasattr(original_attn, "attn_dropout"):
                self.attn_dropout = original_attn.attn_dropout
            if hasattr(original_attn, "resid_dropout"):
                self.resid_dropout = original_attn.resid_dropout
        else:
            for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
                if not hasattr(original_attn, name):
                    avail = [a for a in dir(original_attn) if not a.startswith("_")]
                    raise ValueError(f"Attention module {type(original_attn).__name__} missing "
                                     f"'{name}'. Available attributes: {avail}")
                proj = getattr(original_attn, name)
                if proj is None:
                    raise ValueError(f"'{name}' is None in {type(original_attn).__name__}. "
                                     "This attention implementation may not be compatible.")
                setattr(self, name, proj)
        self.num_heads, self.num_kv_heads, self.head_dim = _get_attention_params(original_attn)
        self.hidden_size = self.num_heads * self.head_dim
        if hasattr(original_attn, "split_size"):
            self.split_size = original_attn.split_size
        self.backend = backend
        self.layer_idx = layer_idx
        self.rotary_emb = rotary_emb
        self.scale = 1.0 / math.sqrt(self.head_dim)

    def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None,
                output_attentions=False, use_cache=False, cache_position=None, layer_past=None,
                head_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, **kwargs):
        if self.model_type == "gpt2":
            return self._forward_gpt2(hidden_states, use_cache=use_cache,
                                      output_attentions=output_attentions)
        return self._forward_llama(hidden_states, position_ids=position_ids)

    def _forward_gpt2(self, hidden_states, use_cache=False, output_attentions=False):
        b, s, _ = hidden_states.shape
        q, k, v = self.c_attn(hidden_states).split(self.split_size, dim=2)
        q = q.view(b, s, self.num_heads, self.head_dim).transpose(1, 2)
        k = k.view(b, s, self.num_kv_heads, self.head_dim).transpose(1, 2)
        v = v.view(b, s, self.num_kv_heads, self.head_dim).transpose(1, 2)
        self._write(k, v, b, s)
        out = self.backend.attend(q, self.layer_idx, seq_id=0)
        out = self.c_proj(out.transpose(1, 2).contiguous().view(b, s, self.hidden_size))
        if hasattr(self, "resid_dropout"):
            out = self.resid_dropout(out)
        outputs = (out, (k, v) if use_cache else None)
        if output_attentions:
            outputs = outputs + (None,)
        return outputs

    def _forward_llama(self, hidden_states, position_ids=None):
        b, s, _ = hidden_states.shape
        q = self.q_proj(hidden_states).view(b, s, self.num_heads, self.head_dim).transpose(1, 2)
        k = self.k_proj(hidden_states).view(b, s, self.num_kv_heads, self.head_dim).transpose(1, 2)
        v = self.v_proj(hidden_states).view(b, s, self.num_kv_heads, self.head_dim).transpose(1, 2)
        if position_ids is None and self.backend.append:
            # the tokens sit behind what this layer already holds of each sequence
            self.backend.check_append_batch(b)
            start = self.backend.manager.ctx_lens[self.layer_idx, :b].to(torch.long)
            position_ids = start.unsqueeze(1) + torch.arange(s, device=hidden_states.device)
            if self.backend._spans is not None:  # ragged: token t of row b sits at start_b + max(t - first_b, 0)
                self.backend._check_spans(b, s)
                first = self.backend._span_buf[:b, 0].to(torch.long)
                position_ids = (position_ids - first.unsqueeze(1)).maximum(start.unsqueeze(1))
        elif position_ids is None:
            position_ids = torch.arange(s, device=hidden_states.device).unsqueeze(0).expand(b, -1)
        cos, sin = self.rotary_emb(v, position_ids)
        q, k = self._apply_rotary_pos_emb(q, k, cos, sin)
        self._write(k, v, b, s)
        out = self.backend.attend(q, self.layer_idx, seq_id=0)
        out = self.o_proj(out.transpose(1, 2).contiguous().view(b, s, self.hidden_size))
        return out, None

    def _write(self, k, v, b, s):
        """backend.write of K/V [b, heads, s, d].  The reference copies them to
        [b, s, heads*d] first (ecc_shim.py:1290-1291, :1351-1352); the fused
        write reads the [b, s, heads, d] views in place."""
        if self.backend._fused_ok(k) and k.dtype == v.dtype:
            self.backend.write(k.transpose(1, 2), v.transpose(1, 2), self.layer_idx, seq_id=0)
        else:
            self.backend.write(k.transpose(1, 2).contiguous().view(b, s, -1),
                               v.transpose(1, 2).contiguous().view(b, s, -1), self.layer_idx,
                               seq_id=0)

    def _apply_rotary_pos_emb(self, q, k, cos, sin):
        def rotate_half(x):
            h = x.shape[-1] // 2
            return torch.cat((-x[..., h:], x[..., :h]), dim=-1)

        q_heads = q.shape[1]
        while cos.dim() < 4:
            cos = cos.unsqueeze(0 if cos.dim() < 2 else 1)
            sin = sin.unsqueeze(0 if sin.dim() < 2 else 1)
        if cos.shape[1] != 1 and cos.shape[1] != q_heads:
            cos, sin = cos[:, :1], sin[:, :1]
        return q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin


def _get_attention_params(attn_module):
    """(num_heads, num_kv_heads, head_dim) of an HF attention module (ecc_shim.py:1556-1611)."""
    cfg = getattr(attn_module, "config", None)
    num_heads = None
    for attr in ("num_heads", "num_attention_heads"):
        if hasattr(attn_module, attr):
            num_heads = getattr(attn_module, attr)
            break
    if num_heads is None and cfg is not None:
        for attr in ("num_attention_heads", "num_heads", "n_head"):
            if hasattr(cfg, attr):
                num_heads = getattr(cfg, attr)
                break
    head_dim = None
    for attr in ("head_dim", "head_size"):
        if hasattr(attn_module, attr):
            head_dim = getattr(attn_module, attr)
            break
    if head_dim is None and cfg is not None:
        if getattr(cfg, "head_dim", None):
            head_dim = cfg.head_dim
        elif hasattr(cfg, "hidden_size") and num_heads:
            head_dim = cfg.hidden_size // num_heads
    num_kv_heads = None
    for attr in ("num_key_value_heads", "num_kv_heads"):
        if hasattr(attn_module, attr):
            num_kv_heads = getattr(attn_module, attr)
            break
    if num_kv_heads is None and cfg is not None:
        for attr in ("num_key_value_heads", "num_kv_heads"):
            if hasattr(cfg, attr):
                num_kv_heads = getattr(cfg, attr)
                break
    if num_kv_heads is None:
        num_kv_heads = num_heads
    if (num_heads is None or head_dim is None) and hasattr(attn_module, "q_proj") and \
            hasattr(attn_module.q_proj, "weight"):
        out_features = attn_module.q_proj.weight.shape[0]
        for cand in (128, 64, 32, 96, 256):
            if out_features % cand == 0:
                head_dim = head_dim or cand
                num_heads = num_heads or out_features // cand
                break
    if num_heads is None:
        raise ValueError("Could not determine num_heads from attention module")
    if head_dim is None:
        raise ValueError("Could not determine head_dim from attention module")
    return num_heads, num_kv_heads, head_dim


def _find_rotary_embedding(model, layers):
    """Locate (or build) the rotary embedding module (ecc_shim.py:1484-1553)."""
    if hasattr(layers[0].self_attn, "rotary_emb"):
        return layers[0].self_attn.rotary_emb
    if hasattr(layers[0], "rotary_emb"):
        return layers[0].rotary_emb
    if hasattr(model, "model") and hasattr(model.model, "rotary_emb"):
        return model.model.rotary_emb
    if hasattr(model, "rotary_emb"):
        return model.rotary_emb
    device = next(model.parameters()).device
    config = getattr(model, "config", None)
    if LlamaRotaryEmbedding is not None and config is not None:
        try:
            return LlamaRotaryEmbedding(config=config, device=device)
        except TypeError:
            pass

    class SimpleRotaryEmbedding(nn.Module):
        def __init__(self, dim, base=10000.0):
            super().__init__()
            inv = 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim))
            self.register_buffer("inv_freq", inv, persistent=False)

        def forward(self, x, position_ids):
            freqs = torch.einsum("i,j->ij", position_ids[0].float(),
                                 self.inv_freq.to(position_ids.device))
            emb = torch.cat((freqs, freqs), dim=-1)
            return emb.cos()[None, None], emb.sin()[None, None]

    _, _, head_dim = _get_attention_params(layers[0].self_attn)
    return SimpleRotaryEmbedding(head_dim).to(device)


@contextmanager
def patch_model_with_ecc_attention(model, config, num_blocks=256):
    """Swap every attention module of an HF model for the ECC shim
    (ecc_shim.py:1395-1481); restored on exit."""
    if hasattr(model, "model") and hasattr(model.model, "layers"):
        layers, model_type = model.model.layers, "llama"
    elif hasattr(model, "layers"):
        layers, model_type = model.layers, "llama"
    elif hasattr(model, "transformer") and hasattr(model.transformer, "h"):
        layers, model_type = model.transformer.h, "gpt2"
    else:
        raise ValueError("Unsupported model architecture")
    attn_attr = "attn" if model_type == "gpt2" else "self_attn"
    num_heads, num_kv_heads, head_dim = _get_attention_params(getattr(layers[0], attn_attr))
    manager = SimpleBlockManager(num_blocks=num_blocks, block_size=config.block_size,
                                 num_layers=len(layers), num_kv_heads=num_kv_heads,
                                 head_dim=head_dim, device=next(model.parameters()).device,
                                 codec=config.codec,
                                 golay_storage=getattr(config, "golay_storage", "int32"))
    backend = ECCBackend(manager, config, num_heads)
    rotary = None if model_type == "gpt2" else _find_rotary_embedding(model, layers)
    originals = {}
    try:
        for i, layer in enumerate(layers):
            originals[i] = getattr(layer, attn_attr)
            setattr(layer, attn_attr, ECCPagedAttentionShim(originals[i], i, backend, rotary,
                                                            model_type))
        model._ecc_block_manager = manager
        model._ecc_backend = backend
        model._ecc_model_type = model_type
        model._ecc_attn_attr = attn_attr
        yield model
    finally:
        for i, orig in originals.items():
            setattr(layers[i], attn_attr, orig)
        for name in ("_ecc_block_manager", "_ecc_backend", "_ecc_model_type", "_ecc_attn_attr"):
            if hasattr(model, name):
                delattr(model, name)


def reset_ecc_cache(model):
    """Fresh cache and counters for a new text (ecc_shim.py:1614-1624); query
    spans held for ragged batches are cleared."""
    if hasattr(model, "_ecc_block_manager"):
        model._ecc_block_manager.reset()
    if hasattr(model, "_ecc_backend"):
        model._ecc_backend.reset_stats()
        model._ecc_backend.set_query_spans(None)


def set_ecc_query_spans(model, counts, firsts=None):
    """Ragged batches in append mode (no reference counterpart): tell the patched
    model which tokens of every following forward's [batch, q_max] rows are real.
    counts / firsts are host integer sequences of length batch -- row b's valid
    tokens are [firsts[b], firsts[b] + counts[b]), firsts defaulting to 0 (right
    padding); kvecc.query_spans_from_mask reads them off an attention mask.
    Padding tokens are not cached and nothing attends to them; a count of 0 holds
    a finished sequence still.  The spans are uploaded once, here, and hold until
    replaced, cleared (counts=None) or reset_ecc_cache.  Pass matching
    position_ids to the model (LLaMA shims derive them when given none)."""
    if not hasattr(model, "_ecc_backend"):
        raise ValueError("model is not patched with patch_model_with_ecc_attention")
    model._ecc_backend.set_query_spans(counts, firsts)


def get_ecc_stats(model):
    """Block and error counters (ecc_shim.py:1627-1642); one device sync."""
    stats = {}
    if hasattr(model, "_ecc_block_manager"):
        m = model._ecc_block_manager
        stats["allocated_blocks"] = sum(sum(1 for x in b if x >= 0) for b in m.seq_to_blocks.values())
        stats["free_blocks"] = len(m.free_blocks)
        stats["sequences"] = len(m.seq_to_blocks)
    if hasattr(model, "_ecc_backend"):
        be = model._ecc_backend
        corrected, detected = be.codec_backend.read_stats(be._stats, 2)
        stats["injection_count"] = be._injection_count
        stats["errors_corrected"] = corrected
        stats["errors_detected"] = detected
        stats["total_values"] = be._total_values
    return stats


def get_ecc_repaired(model):
    """Bytes the repairing attention (ECCShimConfig(repair_attention=True)) has
    rewritten in the resident cache since the last reset_ecc_cache: the sum of
    what a scrub of each layer before each forward would have reported as
    "rewritten".  One device sync; 0 without the flag.  get_ecc_stats does not
    include it."""
    if not hasattr(model, "_ecc_backend"):
        raise ValueError("model is not patched with patch_model_with_ecc_attention")
    be = model._ecc_backend
    if not getattr(be.config, "repair_attention", False):
        return 0
    return be.codec_backend.read_stats(be._stats, 3)[2]


_SCRUB_KEYS = ("corrected", "detected", "rewritten", "scanned")


def scrub_ecc_cache(model, layers=None):
    """Scrub the patched model's resident KV cache in place (no reference
    counterpart; ECCBackend.scrub): every correctable codeword of the cached
    tokens of `layers` (None: all) that differs from its canonical form is
    rewritten, uncorrectable words stay.  Call it between forwards.  Returns this
    call's {"corrected", "detected", "rewritten", "scanned"} (per-codec meaning
    of the first two as get_ecc_stats' errors_corrected / errors_detected; one
    device sync); the counts also add into cumulative scrub counters that
    reset_ecc_cache clears and get_ecc_stats does not include."""
    if not hasattr(model, "_ecc_backend"):
        raise ValueError("model is not patched with patch_model_with_ecc_attention")
    be = model._ecc_backend
    before = be.scrub_totals()
    be.scrub(layers)
    return dict(zip(_SCRUB_KEYS, (int(x) for x in (be.scrub_totals() - before).tolist())))


def evict_ecc_cache(model):
    """Give the blocks that no future query can see under the config's sliding
    window back to the pool (ECCShimConfig(attention_window=W, attention_sinks=S);
    no reference counterpart) and return how many were released.  With Lmin a
    sequence's smallest length over all layers, logical block lb goes iff
    lb * block_size >= S and (lb + 1) * block_size - 1 <= Lmin - W: it is zeroed,
    returned to the sorted free list, and its block-table entry becomes -1, which
    the attention kernels, the scrubber and the batched read all skip.  Call it
    between forwards; ECCShimConfig(evict_blocks=True) does so before every
    forward's first write.  ValueError without a window."""
    if not hasattr(model, "_ecc_backend"):
        raise ValueError("model is not patched with patch_model_with_ecc_attention")
    return model._ecc_backend.evict()


def age_ecc_cache(model, ber, seed):
    """Residency-error model for experiments ("BER p per step, scrub every k
    steps"): flip every bit of the resident K and V cache tensors with
    probability `ber`, in place, with the library's in-place injection (K with
    `seed`, V with `seed + V_SEED_OFFSET`; 7 / 8 / 24 bits per element for hamming74 /
    hamming84 / golay, 8 per byte of the packed Golay layout).  The WHOLE cache
    tensors are aged: unused slots, free blocks and the pad bytes of packed rows
    are flipped too (bit 7 of a hamming74 byte and bits 24..31 of an int32 Golay
    word are not).  The fp32 scales are not touched."""
    if not hasattr(model, "_ecc_backend"):
        raise ValueError("model is not patched with patch_model_with_ecc_attention")
    model._ecc_backend.age(ber, seed)
