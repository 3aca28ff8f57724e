"""Single-token decode steps as ONE captured HIP graph.

An eager decode step of the 4B model is ~900 kernel launches issued from Python: 16.6 ms per token on an MI355X whose
weight-read floor is 1.6 ms (tools/mb_decode.py) -- the step is launch bound, which is what graph capture is for.  To make
a step replayable nothing in it may depend on the current length:
  * the key/value caches have a fixed capacity; the new keys / values land at a device-side position (index_copy_);
  * attention runs over ALL slots through the gathered form (cogv_attn_desc.kv_index); slots not written yet carry the
    masked flag (bit 31) in the index table, which is device data updated between replays;
  * Sandwich-LN's abs-max slots come from a slab at fixed addresses that the graph's first node clears;
  * token and position are read from static device buffers.
Reference path: generation/sampling.py:139-148 (one model call per generated token, layer-input memories)."""
import torch

from .. import functional as F_
from .. import ops
from ..mpu.transformer import KV8Cache, StaticKVSlot


WEIGHT_FORMATS = ("e4m3", "mxfp4")
KV_FORMATS = ("e4m3",)


def unwrap(model):
    while hasattr(model, "module"):
        model = model.module
    return model


MAX_STEP_ROWS = 8          # rows of one decode step: what the skinny products and the chunk attention take


def refuse_unsupported(weights=None, kv=None, ragged=False, args=None, model=None, batch=None, use=None, chunk=0, wide=False,
                       kv_chunk=False):
    """The one rule for what the decode step's options do not cover, applied before anything is allocated or quantized.
    Asked for: weights= / kv= (formats), ragged=True and chunk=C (a second step of C tokens per cache row: 2 <= C <= 8 and
    batch * C <= 8 rows, on the 16-bit cache).  Known, each optional: `args` (a caller's .is_sparse), `model` (its storage
    type), `batch` (the decoder's rows; with it the 8-bit weight stream is put to the kernels' launch plan).  `use`: what the message
    advises instead (a caller's host form; default: the decoder's own plain options).  Sparse generation and model parallelism > 1
    are refused for every caller that hands in `args`, with or without options; a plain decoder refuses nothing.
    wide=True (opt-in; a later change makes it the default): with weights= set, 9 ... 64 rows are put to the wide products' launch
    plan (functional.decode_wide_q_supported) instead of being refused as more than 8 rows.  False: every refusal is what it was.
    kv_chunk=True (opt-in; a later change makes it the default): chunk=C together with kv= is accepted (the chunk step on the 8-bit
    cache, ops.attention_decode_chunk_kv8) under the same limits 2 <= C <= 8 and batch * C <= 8; with kv=None or chunk=0 it does
    nothing.  False: every refusal is what it was."""
    from ..mpu.initialize import mp_world_size_or_1
    if weights is not None and weights not in WEIGHT_FORMATS:
        raise ValueError(f"weights={weights!r}: None (16-bit) or one of {WEIGHT_FORMATS}")
    if kv is not None and kv not in KV_FORMATS:
        raise ValueError(f"kv={kv!r}: None (16-bit cache) or one of {KV_FORMATS}")
    if chunk:
        rows = (batch if batch is not None else 1) * chunk
        if not isinstance(chunk, int) or not 2 <= chunk <= MAX_STEP_ROWS or rows > MAX_STEP_ROWS:
            raise ValueError(f"chunk={chunk!r}: 0 (one-token steps only) or 2 ... {MAX_STEP_ROWS} tokens per cache row with batch * chunk <= "
                             f"{MAX_STEP_ROWS} rows" + (f" (batch {batch})" if batch is not None else ""))
    asked = {name: value for name, value in (("weights", weights), ("kv", kv), ("ragged", ragged or None), ("chunk", chunk or None))
             if value is not None}
    what = " with " + ", ".join(f"{name}={value!r}" for name, value in asked.items()) if asked else ""
    if use is None:
        off = {"ragged": False, "chunk": 0}
        use = ", ".join(f"{name}={off.get(name)}" for name in asked)
    if chunk and kv is not None and not kv_chunk:
        raise NotImplementedError(f"chunk={chunk} with kv={kv!r}: the 8-bit cache quantizes a key before it is attended, so it serves "
                                  f"one-token steps only -- use kv=None")
    if args is not None:
        if args.is_sparse == 2:
            raise NotImplementedError(f"sparse generation (is_sparse = 2){what}: use {use}")
        if args.is_sparse != 0:
            raise ValueError('set is_sparse==2 for inference.')
    if (args is not None or asked) and mp_world_size_or_1() > 1:
        raise NotImplementedError(f"model parallelism > 1{what}: use {use}")
    if model is None or not asked:
        return
    gpt = unwrap(model)
    dt = gpt.word_embeddings.weight.dtype
    # (a caller without the decoder's row count leaves weights= to the decoder, where the transformer is looked at anyway)
    if dt not in (torch.float16, torch.bfloat16) and (kv is not None or ragged or chunk or batch is not None):
        raise NotImplementedError(f"a {dt} model{what}: the 8-bit and 4-bit formats, the per-row `first` slot and the chunk step are the fp16 / bf16 "
                                  f"decode step's -- use {use}")
    if weights is not None and batch is not None:
        if gpt.word_embeddings.weight.shape[0] % 8:
            raise NotImplementedError(f"weights={weights!r}: a vocabulary of {gpt.word_embeddings.weight.shape[0]} rows (not a multiple of 8)")
        for rows in (batch, batch * chunk) if chunk else (batch,):
            if wide and rows > MAX_STEP_ROWS:
                why = F_.decode_wide_q_supported(gpt.transformer, rows, weights)
            else:
                why = (F_.w4_decode_supported if weights == "mxfp4" else F_.w8_decode_supported)(gpt.transformer, rows)
            if why is not None:
                raise NotImplementedError(f"weights={weights!r}: {why}")


class GraphDecoder:
    def __init__(self, model, batch=1, capacity=1152, weights=None, kv=None, ragged=False, chunk=0, wide=False, kv_chunk=False):
        """model: GPT2Model (optionally inside FP16_Module) in eval mode, dense attention; capacity: slots per cache
        (<= 4096, the gathered form's limit).
        weights="e4m3": the decode step streams 8-bit copies of the weights (OCP E4M3 bytes with one fp32 scale per row,
        ops.quantize_rows_e4m3), made here, once: the four Linear weights of every layer and a copy of the word-embedding
        matrix for the tied-logits product -- half the bytes a step reads.  The embedding lookup keeps the 16-bit table and
        the prefill runs on the 16-bit weights (a GEMM, not a stream), so those stay resident: the copies ADD half the
        model's size in device memory (about 4 GB at 4B).  Logits differ from the 16-bit step's by the quantization of the
        weights.  One model-parallel partition, dense attention, fp16 / bf16, hidden sizes whose h and 4h the 8-bit kernels
        cover (the model family's: 1024 and 2560).  None (default): nothing is allocated, the step is what it was.
        weights="mxfp4": the same step on 4-bit copies (OCP MXFP4: E2M1 codes with one E8M0 scale per 32 elements of a row,
        ops.quantize_rows_mxfp4; held as self.w4) -- 0.53 bytes per weight, so the copies add about a quarter of the model's size.
        The format's relative weight error is about four times row-scaled E4M3's (0.114 against 0.026 on Gaussian rows): the
        logits differ from the 16-bit step's accordingly, and nothing is claimed about image quality.  Same limits as "e4m3",
        composes with kv=, ragged= and chunk= the same way.  Measured on the captured 4B step: 2.07 / 2.33 / 2.64 /
        4.09 ms at 1 / 2 / 4 / 8 rows against 2.32 / 2.50 / 2.82 / 4.41 on "e4m3" and 2.79 / 3.21 / 3.66 / 4.91 on 16-bit weights:
        faster than the 8-bit step at every row count.
        kv="e4m3": the key/value caches hold OCP E4M3 bytes with one fp32 scale per (slot, head, K | V) (mpu.transformer.KV8Cache,
        ops.kv_quantize_e4m3 / ops.attention_decode_kv8) INSTEAD of the 16-bit caches: 0.53 of the bytes a step streams from them
        and of their resident memory.  The prefill stays 16-bit; its memories are quantized into the cache.  Logits differ from
        the 16-bit cache's by the quantization of keys and values.  Composes with weights="e4m3".  One model-parallel partition,
        dense attention, fp16 / bf16.  None (default): the 16-bit caches, the step is what it was.
        ragged=True: the cache rows may hold contexts of DIFFERENT lengths (several prompts on one decode step).  Take G
        prompts with context lengths n_g and P = max n_g: row g's context is right-aligned in slots [P - n_g, P), slots
        [0, P - n_g) are padding, and every row writes the same slot *pos_index = P, P + 1, ... -- so the sampler's
        bookkeeping stays shared.  The one new piece of device data is self.first (int32 [batch], zeros): row b attends slots
        [first[b], *pos_index] (cogv_attn_decode_desc.first).  Its address is baked into a capture, so the choice is made
        here.  One model-parallel partition, fp16 / bf16.  False (default): nothing is allocated, the step is what it was.
        chunk=C (2 <= C <= 8, batch * C <= 8): a SECOND step, of C tokens per cache row (step_chunk): rows b * C + j are the tokens
        of slots *pos_index + j, appended to and attended over the same caches by ops.attention_decode_chunk; capture() captures
        it as a second graph.  The Sandwich-LN scale of a chunk step is the abs-max over all its rows, as in a multi-token model
        call, so its logits are not bit-equal to C one-token steps'.  Composes with weights= and ragged=; the 16-bit cache only,
        unless kv_chunk=True.  0 (default): nothing is allocated or captured, the decoder is what it was.
        kv_chunk=True (opt-in; a later change makes it the default): chunk=C together with kv="e4m3" is accepted instead of refused.
        The cache's slots carry the mark StaticKV8Slot.chunk and the chunk step's attention is ops.attention_decode_chunk_kv8: the
        chunk's C keys / values are quantized, stored and attended in their dequantized form, bit for bit what C one-token steps'
        attentions on the same rows leave.  Same limits (2 <= C <= 8, batch * C <= 8); composes with weights= and
        ragged=.  With kv=None or chunk=0 the keyword does nothing.  False (default): every refusal, allocation and launch is
        what it was.
        wide=True (opt-in; a later change makes it the default): with weights= set and 9 ... 64 rows the step runs layer by layer on
        the quantized copies through the wide weight-streaming products (ops.gemm_rows_w8 / ops.gemm_rows_w4; functional.decode_layers(
        wq=..., wide=True)) instead of being refused as more than 8 rows.  Composes with kv= and ragged=; chunk= keeps batch * chunk
        <= 8.  Captured 4B step: 5.13 / 6.87 / 7.85 / 12.75 ms on "e4m3" and 4.91 / 6.71 / 7.74 / 12.63 ms on "mxfp4" at 12 /
        24 / 32 / 64 rows against 5.72 / 7.62 / 8.67 / 13.35 ms on the 16-bit wide step of the same process -- faster at every row
        count measured; against the tile kernels, which the 16-bit decoder takes above 24 rows, not faster from 48 rows on.  With
        16-bit weights, or up to 8 rows, the keyword has no effect.  False (default): every refusal and every launch is what it was."""
        m = unwrap(model)
        self.gpt, tr = m, m.transformer
        assert capacity <= 4096
        self.w8, self.w4, self.kv, self.first = None, None, kv, None
        more = {"kv_chunk": True} if kv_chunk else {}       # handed on only where it is set
        refuse_unsupported(weights, kv, ragged, model=m, batch=batch, chunk=chunk, wide=wide, **more)
        self.chunk = int(chunk)
        if weights == "mxfp4":
            with torch.no_grad():
                self.w4 = F_.W4Weights(tr, m.word_embeddings.weight)
        elif weights is not None:
            with torch.no_grad():
                self.w8 = F_.W8Weights(tr, m.word_embeddings.weight)
        self.wq = self.w4 if self.w4 is not None else self.w8       # the quantized copies the step streams, if any
        self.wide_q = bool(wide) and self.wq is not None and batch > MAX_STEP_ROWS      # the step takes the wide products on them
        p0 = tr.layers[0].attention.query_key_value.weight
        hp = tr.layers[0].attention.hidden_size_per_partition
        dev, dt = p0.device, p0.dtype
        self.batch, self.cap, self.length = batch, capacity, 0
        self.tok = torch.zeros((batch, 1), dtype=torch.long, device=dev)
        self.pos = torch.zeros((batch, 1), dtype=torch.long, device=dev)
        self.pos_index = torch.zeros(1, dtype=torch.long, device=dev)
        self.table = torch.arange(capacity, dtype=torch.int64, device=dev)
        self.masked = ((self.table | (1 << 31)) - (1 << 32)).to(torch.int32)       # every slot flagged: nothing visible
        self.table = self.masked.unsqueeze(0).repeat(batch, 1).contiguous()
        if ragged:
            self.first = torch.zeros(batch, dtype=torch.int32, device=dev)
        if kv is None:
            self.kv8 = None
            self.caches = [torch.zeros((batch, capacity, 2 * hp), dtype=dt, device=dev) for _ in tr.layers]
            self.slots = [StaticKVSlot(c, self.pos_index, self.table, self.first) for c in self.caches]
        else:
            more = {"chunk": True} if kv_chunk and self.chunk else {}       # the slots' mark for chunk steps
            self.kv8 = KV8Cache(len(tr.layers), batch, hp // 64, capacity, self.pos_index, dev, self.first, **more)
            self.caches, self.slots = None, self.kv8.slots
        self.slab = torch.zeros(8 * len(tr.layers) + 16, dtype=torch.float32, device=dev)
        self.graph, self.logits = None, None
        self.fused = True            # False: layer-by-layer path (every LayerNorm its own launch) -- kept for comparison
        if self.chunk:
            self.tok_chunk = torch.zeros((batch, self.chunk), dtype=torch.long, device=dev)
            self.pos_chunk = torch.zeros((batch, self.chunk), dtype=torch.long, device=dev)
            self.chunk_j = torch.arange(self.chunk, dtype=torch.long, device=dev)
            self.graph_chunk, self.logits_chunk = None, None

    # ------------------------------------------------------------------ one decode step, eager (also what gets captured)
    def _step(self):
        tr = self.gpt.transformer
        self.slab.zero_()
        with ops.scalar_slab(self.slab):
            h = tr.embed(self.tok, self.pos, self.gpt.word_embeddings)
            if self.fused and F_.decode_chain_supported(tr, self.batch):
                # five launches per layer: the LayerNorms ride as prologues of the GEMVs, the cache append inside the
                # decode attention kernel (functional.decode_chain); w8: the same chain on the 8-bit copies of the weights
                return F_.decode_chain(tr, h, h._cogv_absmax, self.slots, self.gpt.word_embeddings.weight, wq=self.wq)
            if self.wide_q:
                # 9 .. 64 rows on the quantized copies: the five products as weight streams (ops.gemm_rows_w8 / ops.gemm_rows_w4)
                return F_.decode_layers(tr, h, h._cogv_absmax, self.slots, None, wq=self.wq, wide=True)
            if self.wq is not None:
                return F_.decode_layers(tr, h, h._cogv_absmax, self.slots, None, wq=self.wq)
            if F_.decode_wide_supported(tr, self.batch):
                # 9 .. 64 rows on the 16-bit weights: layer by layer, the five products as weight streams (ops.gemm_rows)
                return F_.decode_layers(tr, h, h._cogv_absmax, self.slots, self.gpt.word_embeddings.weight, wide=True)
            for layer, slot in zip(tr.layers, self.slots):
                h = layer(h, 0, mem=slot)
            out = tr.final_layernorm(h)
            return F_.tied_logits(out, self.gpt.word_embeddings.weight)

    def _step_chunk(self):
        """One step of `chunk` tokens per cache row, eager (also what gets captured): the chain up to
        COGV_DECODE_CHAIN_MAX_ROWS rows, above it layer by layer.  Returns logits [batch, chunk, vocab]."""
        tr = self.gpt.transformer
        self.slab.zero_()
        with ops.scalar_slab(self.slab):
            h = tr.embed(self.tok_chunk, self.pos_chunk, self.gpt.word_embeddings)
            if self.fused and F_.decode_chain_supported(tr, self.batch * self.chunk):
                return F_.decode_chain(tr, h, h._cogv_absmax, self.slots, self.gpt.word_embeddings.weight, wq=self.wq)
            return F_.decode_layers(tr, h, h._cogv_absmax, self.slots, self.gpt.word_embeddings.weight, wq=self.wq)

    def capture(self):
        """Warm up on a side stream (first-use allocations inside the library and the caching allocator), then capture."""
        assert 0 < self.length < self.cap, "prefill first: the warm-up steps write at the current position"
        self.pos_index.fill_(self.length)     # warm-up and capture runs scribble on the next (still masked) slot only
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(3):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.logits = self._step()
        if self.chunk:
            self._capture_chunk()

    def _capture_chunk(self):
        """The chunk step as a second graph (its warm-up and capture runs scribble on the next `chunk` slots, none past the capacity)."""
        self.pos_index.fill_(self.length)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(3):
                self._step_chunk()
        torch.cuda.current_stream().wait_stream(s)
        self.graph_chunk = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph_chunk):
            self.logits_chunk = self._step_chunk()

    # ------------------------------------------------------------------ cache management (outside the graph)
    @torch.no_grad()
    def prefill(self, tokens, position_ids, attention_mask=0):
        """Run the context through the model once (eager, K/V-cache memories) and load the caches.  Returns its logits."""
        assert tokens.shape[0] == self.batch
        return self._prefill(tokens, position_ids, attention_mask)

    def _prefill(self, tokens, position_ids, attention_mask, pads=None):
        """prefill's body; tokens of ONE row fill every cache row (the keys / values broadcast over the batch).
        pads (ragged=True; attention_mask is not read): G prompts of different lengths, tokens / position_ids [G, P], every prompt
        right-aligned (row g's ids in columns [pads[g], P)); the padding columns are overwritten here with a real id (the row's
        first token) and position 0.  One model call under the mask M[g, i, j] = (j <= i) and (j >= pads[g]) (the general-mask
        attention path: prompt-length work); the memories of prompt g fill its batch // G cache rows, first[b] = pads[g] keeps the
        padding slots out of every later step.  Returns the logits [rows of tokens, n, vocab]."""
        G, n = tokens.shape
        assert n < self.cap
        dev, nb = self.table.device, 1
        if pads is None:
            assert G in (1, self.batch)
        else:
            assert self.first is not None, "built without ragged=True"
            assert len(pads) == G and self.batch % G == 0 and n > 0 and all(0 <= p < n for p in pads)
            nb = self.batch // G
            pad_t = torch.tensor(list(pads), dtype=torch.long, device=dev)
            col = torch.arange(n, dtype=torch.long, device=dev)
            is_pad = col.unsqueeze(0) < pad_t.unsqueeze(1)                                            # [G, n]
            tokens = torch.where(is_pad, tokens.gather(1, pad_t.unsqueeze(1)).expand(G, n), tokens)
            position_ids = position_ids.masked_fill(is_pad, 0)
            attention_mask = ((col.view(1, 1, n) <= col.view(1, n, 1)) & (col.view(1, 1, n) >= pad_t.view(G, 1, 1))).float().unsqueeze(1)
        tr = self.gpt.transformer
        kv_flag, tr.kv_cache = tr.kv_cache, True
        max_mem, tr.max_memory_length = tr.max_memory_length, max(tr.max_memory_length, self.cap)
        try:
            logits, *mems = self.gpt(tokens, position_ids, attention_mask, None, None, 0)
        finally:
            tr.kv_cache, tr.max_memory_length = kv_flag, max_mem
        for slot, mem in zip(self.slots, mems):           # 1 or B rows; row g * nb + j: candidate j of prompt g
            slot.load(mem.repeat_interleave(nb, 0) if nb > 1 else mem)
        if pads is None:
            self.table[:, :n] = torch.arange(n, dtype=torch.int32, device=dev)
        else:
            first = pad_t.repeat_interleave(nb).to(torch.int32)
            self.first.copy_(first)
            # (the op-by-op step reads the table: the padding slots stay flagged)
            self.table[:, :n] = torch.where(col.unsqueeze(0) < first.unsqueeze(1), self.masked[:n].unsqueeze(0), col.to(torch.int32).unsqueeze(0))
        self.table[:, n:] = self.masked[n:]           # a longer earlier run left these visible (the op-by-op step reads them)
        self.length = n
        return logits

    def _replay_or_step(self):
        """One decode step: a replay of the captured graph, else the same launches eagerly.  Returns the logits."""
        if self.graph is None:
            return self._step()
        self.graph.replay()
        return self.logits

    @torch.no_grad()
    def step(self, token, position):
        """token, position: [batch, 1] (or [batch]) device tensors for the next input.  Returns logits [batch, 1, vocab]
        (a static buffer when the step is captured: consume it before the next call)."""
        assert self.length < self.cap, "key/value cache capacity exhausted"
        self.tok.copy_(token.view(self.batch, 1))
        self.pos.copy_(position.view(self.batch, 1))
        self.pos_index.fill_(self.length)
        self.table[:, self.length] = self.length          # this step's own slot becomes visible
        logits = self._replay_or_step()
        self.length += 1
        return logits

    def _replay_or_step_chunk(self):
        if self.graph_chunk is None:
            return self._step_chunk()
        self.graph_chunk.replay()
        return self.logits_chunk

    @torch.no_grad()
    def step_chunk(self, tokens, positions):
        """tokens, positions: [batch, chunk] device tensors -- the next `chunk` inputs of every row.  Returns logits [batch, chunk,
        vocab] (a static buffer when captured): row j's are those of the one-token step that fed tokens[:, j]."""
        assert self.chunk, "built without chunk="
        C = self.chunk
        assert self.length + C <= self.cap, "key/value cache capacity exhausted"
        self.tok_chunk.copy_(tokens.view(self.batch, C))
        self.pos_chunk.copy_(positions.view(self.batch, C))
        self.pos_index.fill_(self.length)
        self.table[:, self.length:self.length + C] = torch.arange(self.length, self.length + C, dtype=torch.int32, device=self.table.device)
        logits = self._replay_or_step_chunk()
        self.length += C
        return logits


class SamplingDecoder(GraphDecoder):
    """A GraphDecoder whose step ends with the token sampler (ops.sample_logits, cogv_sample_logits): the drawn ids go
    straight into the static token buffer, and the same launch advances the positions, the write slot, the visible slot of
    the index table, the generator offset and the output row -- so one replay of the captured graph is one generated token
    and a run of them needs no host work.  Reference path: generation/sampling.py:139-186 (model call, filter, multinomial,
    beam score) once per token.  Use start() + generate() (step() feeds tokens from the host and is not for this mode)."""

    def __init__(self, model, batch=1, capacity=1152, weights=None, kv=None, ragged=False, chunk=0, wide=False, kv_chunk=False):
        """chunk=C: generate(n, widths=...) may feed runs of given ids as chunk steps (GraphDecoder's `chunk`; _step_chunk below).
        wide: GraphDecoder's (opt-in: quantized weights at 9 ... 64 rows).  kv_chunk: GraphDecoder's (opt-in; a later change makes
        it the default: chunk=C on the 8-bit cache)."""
        more = {"kv_chunk": True} if kv_chunk else {}
        super().__init__(model, batch, capacity, weights=weights, kv=kv, ragged=ragged, chunk=chunk, wide=wide, **more)
        self.sampling = None
        self.chunk_steps = 0         # chunk steps run by generate() so far

    def enable_sampling(self, temperature=1.0, top_k=0, top_p=0.0, allow=None, seed=0, out_tokens=None, out_base=0,
                        given=None):
        """allow: (lo, hi) range of ids that may be drawn (None: all); out_tokens: int64 [batch, n] that receives the id
        drawn for sequence position out_base + j in column j (None: not recorded); given: int64 [capacity] device buffer,
        by sequence position, of ids to feed instead of drawing (-1: draw), shared by all rows -- device data, so one
        captured graph serves any table written into it (None: every position is drawn).  Or int64 [batch, capacity]: one
        table per row, by slot (several images on one ragged decoder: row b is fed where given[b, slot] >= 0; chunk steps need
        the same slots given in every row)."""
        dev = self.tok.device
        assert out_tokens is None or (out_tokens.dtype == torch.int64 and out_tokens.shape[0] == self.batch)
        assert given is None or (given.dtype == torch.int64 and given.shape[-1] >= self.cap and given.device == dev)
        assert given is None or given.dim() == 1 or (given.dim() == 2 and given.shape[0] == self.batch and given.stride(1) == 1)
        self.sampling = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), allow=allow, seed=int(seed))
        self.offset = torch.zeros(1, dtype=torch.int64, device=dev)        # generator offset: one per draw
        self.ids = torch.zeros(self.batch, dtype=torch.int64, device=dev)
        self.logp = torch.zeros(self.batch, dtype=torch.float32, device=dev)
        self.scores = torch.zeros(self.batch, dtype=torch.float32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)       # the sampler's completion counter
        self.out_tokens, self.out_base, self.given = out_tokens, int(out_base), given

    def _sample(self, logits, rows=None):
        dec = dict(tok=self.tok.view(-1), pos=self.pos.view(-1), pos_index=self.pos_index, table=self.table,
                   counter=self.counter, out_tokens=self.out_tokens, out_base=self.out_base, given=self.given)
        ops.sample_logits(logits, **self.sampling, offset=self.offset, rows=rows, ids=self.ids, logp=self.logp,
                          scores=self.scores, decode=dec)

    def _step(self):
        logits = super()._step()
        if self.sampling is not None:
            self._sample(logits)
        return logits

    def _step_chunk(self):
        """A chunk step inside a sampling run, all on the device: row 0 is the token the previous step published, rows 1 ... C - 1 are
        the given ids of the next C - 1 positions (the plan guarantees they are set; the clamps only keep a warm-up run at the end
        of the cache inside the tables); with a table per row, each row's own.  After the layers the decoder state is advanced by
        C - 1 -- what C - 1 one-token steps that fed a given id would have left: write slot, positions, generator offset (one per position in both modes), the visible
        slots, the output columns -- and the unchanged sampler runs on the last row's logits, exactly as if the one-token step at
        that position had just run."""
        if self.sampling is None:
            return super()._step_chunk()
        assert self.given is not None, "chunk steps inside a sampling run feed given ids: enable_sampling(given=...)"
        C, j = self.chunk, self.chunk_j
        at = self.pos_index + j                                                            # sequence positions of the chunk's rows
        self.tok_chunk[:, :1].copy_(self.tok)
        if self.given.dim() == 1:
            self.tok_chunk[:, 1:].copy_(self.given.index_select(0, at[1:].clamp(max=self.cap - 1)).clamp(min=0).unsqueeze(0).expand(self.batch, C - 1))
        else:                                                                              # every row's own ids
            self.tok_chunk[:, 1:].copy_(self.given.index_select(1, at[1:].clamp(max=self.cap - 1)).clamp(min=0))
        max_pos = self.gpt.transformer.position_embeddings.weight.shape[0] - 1
        self.pos_chunk.copy_((self.pos + j).clamp(max=max_pos))
        logits = super()._step_chunk()
        p0 = self.pos_index.clone()
        slots = torch.arange(self.cap, dtype=torch.long, device=p0.device)
        new = (slots > p0) & (slots < p0 + C)                                              # positions p0 + 1 ... p0 + C - 1
        self.table.copy_(torch.where(new.unsqueeze(0), slots.to(torch.int32).unsqueeze(0), self.table))
        if self.out_tokens is not None:
            cols = torch.arange(self.out_tokens.shape[1], dtype=torch.long, device=p0.device) + self.out_base
            if self.given.dim() == 1:
                fed = self.given.index_select(0, cols.clamp(0, self.cap - 1)).unsqueeze(0)
            else:
                fed = self.given.index_select(1, cols.clamp(0, self.cap - 1))
            self.out_tokens.copy_(torch.where(((cols > p0) & (cols < p0 + C)).unsqueeze(0), fed, self.out_tokens))
        self.pos_index.add_(C - 1)
        self.pos.add_(C - 1)
        self.offset.add_(C - 1)
        self._sample(logits[:, -1])
        return logits

    def _first_draw(self, last_pos, last_logits, rows=None):
        """The tail of start / start_ragged after the prefill: every row's first token is drawn from its prompt's last logits, and
        the draw's bookkeeping leaves the decoder at the next step."""
        self.pos_index.fill_(self.length - 1)
        self.pos.copy_(last_pos)
        self.scores.zero_()
        self._sample(last_logits, rows=rows)

    @torch.no_grad()
    def start(self, tokens, position_ids, attention_mask=0):
        """Prefill ONE context row [1, n] into every cache row, then draw the first token of every row from its last
        logits (batch independent draws, multinomial(..., replacement=True) in the reference).  The draw's bookkeeping
        leaves the decoder at the next step: slot n visible, the drawn ids and positions in the static buffers."""
        assert self.sampling is not None and tokens.shape[0] == 1
        logits = self._prefill(tokens, position_ids, attention_mask)
        self._first_draw(position_ids[:, -1:].expand(self.batch, 1), logits[:, -1], rows=self.batch)
        return logits

    @torch.no_grad()
    def start_ragged(self, tokens, position_ids, pads):
        """start() for G prompts (ragged=True): tokens / position_ids [G, P] right-aligned, pads[g] padding columns in front of
        prompt g (_prefill's pads).  Every prompt's last logits draw the first token of its batch // G rows -- the rows are
        repeated, so the sampler reads [batch, vocab] with a real row stride -- and every row's position counts on from its
        own prompt's last position id."""
        assert self.sampling is not None
        logits = self._prefill(tokens, position_ids, None, pads)
        nb = self.batch // tokens.shape[0]
        self._first_draw(position_ids[:, -1:].repeat_interleave(nb, 0), logits[:, -1].repeat_interleave(nb, 0))
        return logits

    def capture(self):
        """GraphDecoder.capture, with the state the warm-up steps advance (tokens, positions, table, generator offset,
        scores, output row) restored afterwards."""
        state = [t.clone() for t in self._state()]
        super().capture()
        for t, s in zip(self._state(), state):
            t.copy_(s)

    def _state(self):
        st = [self.tok, self.pos, self.pos_index, self.table, self.offset, self.ids, self.logp, self.scores]
        return st + ([self.out_tokens] if self.out_tokens is not None else [])

    @torch.no_grad()
    def generate(self, n, widths=None):
        """n decode steps back to back (graph replays when captured, else the same launches eagerly): n more tokens per
        row.  Returns (out_tokens, scores) -- device tensors; nothing is read back on the way.
        widths (plan_chunk_steps; a decoder built with chunk=C): the n positions as model calls of width 1 (the one-token step) or
        C (the chunk step: its C - 1 later inputs are given ids); they sum to n."""
        assert self.sampling is not None and self.length + n <= self.cap, "key/value cache capacity exhausted"
        if widths is None:
            for _ in range(n):
                self._replay_or_step()
        else:
            assert sum(widths) == n and all(w == 1 or (self.chunk and w == self.chunk) for w in widths)
            for w in widths:
                if w == 1:
                    self._replay_or_step()
                else:
                    self._replay_or_step_chunk()
                    self.chunk_steps += 1
        self.length += n
        return self.out_tokens, self.scores
