"""Autoregressive filling of a token sequence with memories -- the reference's generation/sampling.py:25-209 on the
HIP model.  Host logic (filtering, sampling, beam bookkeeping) is torch; the model calls are the HIP path.  With
`GPT2Model(..., kv_cache=True)` the memories are per-layer key/value caches appended in place, so a step costs the new
positions only; with the reference's layer-input memories the same loop works unchanged (the K/V of the whole memory are
re-projected every step, as in mpu/sparse_transformer.py:135-140).

`seq`: 1-D tensor; ids >= 0 are given, -1 = generate one token, -N = generate with N beams.
`args`: object with .temperature, .top_k, .top_p, .is_sparse (0 or 2).
`tokenizer`: anything with the unified tokenizer's id-space interface (default: IdSpace(), the released layout)."""
import torch
import torch.nn.functional as F

from . import decoder
from .id_space import IdSpace


def top_k_logits(logits, top_k=0, top_p=0.0, filter_value=-float('Inf')):
    """generation/sampling.py:25-50: keep the top_k largest logits and/or the smallest set whose probability mass
    exceeds top_p (the nucleus form works on one row, as in the reference)."""
    if top_k > 0:
        kth = torch.topk(logits, top_k)[0][..., -1, None]
        logits[logits < kth] = filter_value
    if top_p > 0.0:
        row = logits.view(logits.size()[1]).contiguous()
        sorted_logits, sorted_indices = torch.sort(row, descending=True)
        cumulative = torch.cumsum(F.softmax(sorted_logits, dim=-1), dim=-1)
        remove = cumulative > top_p
        remove[..., 1:] = remove[..., :-1].clone()      # keep the first token that crosses the threshold
        remove[..., 0] = 0
        row[sorted_indices[remove]] = filter_value
        logits = row.view(1, -1).contiguous()
    return logits


def get_batch(context_tokens, device, args=None):
    """generation/sampling.py:52-63 with pretrain_gpt2.get_masks_and_position_ids (:265-299) for the plain case:
    left-to-right mask [1, 1, s, s] and positions 0..s-1."""
    tokens = context_tokens
    tokens = tokens.unsqueeze(0).contiguous() if tokens.dim() == 1 else tokens.view(tokens.shape[0], -1).contiguous()
    tokens = tokens.to(device)
    s = tokens.shape[1]
    attention_mask = torch.tril(torch.ones((1, s, s), device=device)).unsqueeze(1)
    position_ids = torch.arange(s, dtype=torch.long, device=device).unsqueeze(0).expand_as(tokens).clone()
    return tokens, attention_mask, position_ids


def shrink_beams(tokens, mems, nb, score):
    """generation/sampling.py:188-198: fall back to the best beam when the beam count changes."""
    if tokens.shape[0] == nb:
        return tokens, mems, score
    max_idx = score.index(max(score))
    return tokens[max_idx].unsqueeze(0), [mem[max_idx: max_idx + 1] for mem in mems], [0]


def add_interlacing_beam_marks(seq, nb=12, period=3000):
    """generation/sampling.py:200-211: turn runs of -1 into -nb, alternating the beam count every `period` tokens."""
    assert isinstance(seq, list) or len(seq.shape) == 1
    blk_cnt = 0
    for i in range(len(seq)):
        if seq[i] == -1:
            blk_cnt += 1
            seq[i] = -nb
            if blk_cnt == period:
                nb += (nb % 2) * 2 - 1
                blk_cnt = 0
        else:
            blk_cnt = 0


def _slices_after(tok, current, n_img, n_txt, boi, eoi):
    """The ids a marker forbids from the next position on (generation/sampling.py:88-95, 107-114)."""
    if tok in boi:                                     # inside an image: only image codes may be generated
        return [slice(n_img, None)]
    if tok in eoi:                                     # after an image: only text pieces
        return [slice(0, n_img), slice(n_img + n_txt, None)]
    return current


def filling_sequence(model, seq, args, mems=None, invalid_slices=[], tokenizer=None, **kwargs):
    """generation/sampling.py:65-186.  Returns the completed token rows [beams, len(seq)]."""
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    n_img, n_txt = tokenizer.img_tokenizer.num_tokens, tokenizer.txt_tokenizer.num_tokens
    boi, eoi = (tokenizer['[BOI1]'], tokenizer['[BOI2]']), (tokenizer['[EOI1]'], tokenizer['[EOI2]'])
    roi2 = tokenizer['[ROI2]']
    device = seq.device
    assert len(seq.shape) == 1
    out_seq_length = len(seq)
    seq_l = seq.tolist()                              # one host copy instead of a device sync per comparison
    context_length, offset = 0, 100000
    invalid_slices = [slice(0, n_img)]

    def slices_after(tok, current):
        return _slices_after(tok, current, n_img, n_txt, boi, eoi)

    while seq_l[context_length] >= 0:
        invalid_slices = slices_after(seq_l[context_length], invalid_slices)
        if seq_l[context_length] == roi2:
            offset = context_length
        context_length += 1
    tokens, attention_mask, position_ids = get_batch(seq[:context_length], device, args)
    counter, index = context_length - 1, 0
    mems = [] if mems is None else mems
    score = [0]
    if args.is_sparse == 2:
        img_indices_bool = tokens < n_img
        txt_indices_bool = ~img_indices_bool
    elif args.is_sparse == 0:
        txt_indices_bool = img_indices_bool = None
    else:
        raise ValueError('set is_sparse==2 for inference.')

    with torch.no_grad():
        while counter < out_seq_length - 1:
            nxt = seq_l[counter + 1]
            invalid_slices = slices_after(nxt, invalid_slices)
            if index == 0:                                                     # the whole context at once
                position_ids[position_ids > offset] -= offset
                logits, *mems = model(tokens, position_ids, attention_mask, txt_indices_bool, img_indices_bool,
                                      args.is_sparse, *mems)
                index = counter
            elif nxt >= 0:                                                      # a given token: just append it
                if nxt == roi2:
                    offset = counter + 1
                tokens, mems, score = shrink_beams(tokens, mems, 1, score)
                counter += 1
                tokens = torch.cat((tokens, seq[counter: counter + 1].expand(tokens.shape[0], 1)), dim=1)
                if args.is_sparse == 2:
                    img_indices_bool = tokens < n_img
                    txt_indices_bool = ~img_indices_bool
                continue
            else:
                assert tokens.shape[1] == counter + 1
                position_ids = torch.arange(index, counter + 1, dtype=torch.long, device=device).unsqueeze(0)
                position_ids[position_ids > offset] -= offset
                tokens, mems, score = shrink_beams(tokens, mems, -nxt, score)
                logits, *mems = model(tokens[:, index:], position_ids, 0, txt_indices_bool, img_indices_bool,
                                      args.is_sparse, *mems)
                index = counter
            nb = -nxt
            counter += 1
            index += 1

            logits = logits[:, -1].float()                                      # [beams, vocab]
            logits /= args.temperature
            for invalid_slice in invalid_slices:
                logits[..., invalid_slice] = -float('Inf')
            logits = top_k_logits(logits, top_k=args.top_k, top_p=args.top_p)
            probs = F.softmax(logits, dim=-1)
            if nb > 1 and tokens.shape[0] == 1:                                 # 1 -> nb beams
                tokens = tokens.expand(nb, -1).contiguous()
                mems = [mem.expand(nb, -1, -1) for mem in mems]
                prev = torch.multinomial(probs, num_samples=nb, replacement=True)
                score = torch.log(torch.gather(probs, dim=1, index=prev)[0]).tolist()
            else:                                                               # nb -> nb
                assert tokens.shape[0] == nb
                prev = torch.multinomial(probs, num_samples=1)
                score_plus = torch.log(torch.gather(probs, dim=1, index=prev)[:, 0])
                for idx in range(nb):
                    score[idx] += score_plus[idx]
            tokens = torch.cat((tokens, prev.view(tokens.shape[0], 1)), dim=1)
            if args.is_sparse == 2:
                img_indices_bool = tokens < n_img
                txt_indices_bool = ~img_indices_bool
    return tokens.view(tokens.shape[0], -1).contiguous()


def inverse_prompt_score(model, seq, args, tokenizer=None):
    """generation/sampling.py:222-239 (post-selection): for rows laid out as [BASE] [BOI1] 1024 image codes [EOI1] [ROI1] text...,
    the log-likelihood of the text given the image -- one full forward per call, image codes excluded from the softmax,
    summed over the text positions.  Returns [rows] fp32."""
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    assert seq.dim() == 2
    first_text = 2 + 1024 + 1                                   # index of [ROI1]: the text it scores starts right after
    assert int(seq[0, first_text]) == tokenizer['[ROI1]']
    tokens, attention_mask, position_ids = get_batch(seq, seq.device, args)
    with torch.no_grad():
        logits, *_ = model(tokens, position_ids, attention_mask, None, None, args.is_sparse)
        logits = logits.float()
        logits[..., :tokenizer.img_tokenizer.num_tokens] = -float('Inf')
        log_probs = F.log_softmax(logits[:, first_text:-1], dim=-1)
        return torch.gather(log_probs, 2, tokens[:, first_text + 1:].unsqueeze(-1)).squeeze(-1).sum(dim=-1)


def _score_chunks(num, max_rows):
    """The row blocks one scoring forward takes each, by the rule of the reference's post_selection loop
    (generate_samples.py:254-259): `num < mbz or num % mbz == 0`, then max(num // mbz, 1) blocks of mbz rows."""
    if max_rows is None:
        return [(0, num)]
    mbz = int(max_rows)
    if mbz <= 0:
        raise ValueError(f"max_rows = {max_rows} must be positive")
    if not (num < mbz or num % mbz == 0):
        raise ValueError(f"{num} rows are neither fewer than max_rows = {mbz} nor a multiple of it (the reference's post_selection rule)")
    return [(i * mbz, min((i + 1) * mbz, num)) for i in range(max(num // mbz, 1))]


def inverse_prompt_score_on_device(model, seq, args, tokenizer=None, image_tokens=1024, max_rows=None):
    """inverse_prompt_score with the softmax tail on the device (ops.score_targets, cogv_score_targets): same rows
    ([BASE] [BOI1] image_tokens codes [EOI1] [ROI1] text...), same meaning, same result ([rows] fp32).  Embedding and
    transformer run as in GPT2Model.forward; the hidden states are cut to the T text-predicting positions ([ROI1] .. L - 2)
    BEFORE the tied output projection, so the logits are [rows, T, vocab] in the storage type -- no product over the image
    positions, no fp32 copy -- and one launch scores them with the image codes excluded.  [ROI1] is checked in every row
    (one comparison, one read-back).  max_rows: rows per forward (default: args.max_inference_batch_size when present, else
    all), by the reference's post_selection rule.  Dense attention and one model-parallel partition; sparse (is_sparse = 2)
    and model parallelism > 1 are inverse_prompt_score's."""
    from .. import functional as F_
    from .. import ops
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    decoder.refuse_unsupported(args=args, use="inverse_prompt_score")
    assert seq.dim() == 2
    first_text = 2 + image_tokens + 1                            # index of [ROI1]: the text it scores starts right after
    n_text = seq.shape[1] - 1 - first_text
    if n_text < 1:
        raise ValueError(f"rows of {seq.shape[1]} ids hold no text after [ROI1] (index {first_text}): nothing to score")
    if bool((seq[:, first_text] != tokenizer['[ROI1]']).any()):
        raise ValueError(f"[ROI1] is not at index {first_text} of every row")
    if max_rows is None:
        max_rows = getattr(args, "max_inference_batch_size", None)
    gpt = decoder.unwrap(model)
    vocab = gpt.word_embeddings.weight.shape[0]
    scores = torch.empty(seq.shape[0], dtype=torch.float32, device=seq.device)
    with torch.no_grad():
        for lo, hi in _score_chunks(seq.shape[0], max_rows):
            tokens, attention_mask, position_ids = get_batch(seq[lo:hi], seq.device, args)
            h0 = gpt.transformer.embed(tokens, position_ids, gpt.word_embeddings)
            hL, *_ = gpt.transformer(h0, position_ids, attention_mask, None, None, 0, embedded=True)
            logits = F_.tied_logits(hL[:, first_text:-1], gpt.word_embeddings.weight)
            ops.score_targets(logits, tokens[:, first_text + 1:], allow=(tokenizer.img_tokenizer.num_tokens, vocab),
                              group=n_text, scores=scores[lo:hi])
    return scores


def post_selection_rows(tokens, tokenizer, image_tokens=1024):
    """Completed text-to-image rows [nb, L] laid out [ROI1] text... [BASE] [BOI1] codes... (what generate_on_device and
    filling_sequence return) -> the rows inverse_prompt_score reads, [nb, 2 + image_tokens + 1 + 1 + len(text)] laid out
    [BASE] [BOI1] codes [EOI1] [ROI1] text... (the reference's '[BASE] [BOI1] [Image]{} [EOI1] [ROI1] {}' template).  Tensor
    ops on the rows' device, one read-back for the layout check."""
    if tokens.dim() != 2 or tokens.shape[1] < image_tokens + 3:
        raise ValueError(f"want rows [nb, 1 + len(text) + 2 + {image_tokens}], got {tuple(tokens.shape)}")
    n = tokens.shape[1] - image_tokens                          # [ROI1] text [BASE] [BOI1]
    head, codes = tokens[:, :n], tokens[:, n:]
    ok = (head[:, 0] == tokenizer['[ROI1]']) & (head[:, n - 2] == tokenizer['[BASE]']) & (head[:, n - 1] == tokenizer['[BOI1]'])
    ok = ok.all() & (codes >= 0).all() & (codes < tokenizer.img_tokenizer.num_tokens).all()
    if not bool(ok):
        raise ValueError(f"rows are not [ROI1] text [BASE] [BOI1] followed by {image_tokens} image codes")
    mid = torch.tensor([tokenizer['[EOI1]'], tokenizer['[ROI1]']], dtype=tokens.dtype, device=tokens.device)
    return torch.cat((head[:, n - 2:], codes, mid.expand(tokens.shape[0], 2), head[:, 1:n - 2]), dim=1)


def rerank_generated(model, tokens, args, tokenizer=None, image_tokens=1024, keep=None, max_rows=None):
    """Post-selection of generated candidates: the text-to-image rows of generate_on_device / filling_sequence, best first
    by how well each image predicts its caption (inverse_prompt_score_on_device of post_selection_rows).  Returns
    (tokens[order][:keep], scores[order][:keep], order[:keep]); `order` is a stable descending sort (-inf rows last),
    everything stays on the device.  A returned row feeds magnify as it is: row[-image_tokens:] are the codes,
    row[1:n - 2] (n = len(row) - image_tokens) the text."""
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    scores = inverse_prompt_score_on_device(model, post_selection_rows(tokens, tokenizer, image_tokens), args, tokenizer=tokenizer,
                                            image_tokens=image_tokens, max_rows=max_rows)
    order = torch.sort(scores, descending=True, stable=True)[1]
    if keep is not None:
        order = order[:int(keep)]
    return tokens[order], scores[order], order


# (row block, column block, lines to fill) of the nine overlapping 16 x 16 -> 32 x 32 windows, in generation order
_MAGNIFY_WINDOWS = ((0, 0, 18), (0, 1, 30), (0, 2, 30), (1, 1, 30), (1, 0, 30), (1, 2, 30), (2, 0, 32), (2, 1, 32), (2, 2, 32))


def magnify(model, tokenizer, tokens_list, text_token_list, args, fill=None):
    """generation/magnify.py:22-43 (super-resolution): a 32 x 32 code map is magnified to 64 x 64 window by window -- each window
    conditions on the text, a 16 x 16 patch of the small map and the marker run [EOI1] [ROI2] [POS0] [BASE] [BOI2], and fills
    the not-yet-written lines of the matching 32 x 32 patch of the large map (lines written by an earlier window are given).
    Returns [1, 4096] codes.  `fill`: the sequence filler (default: filling_sequence of this module; the tokenizer is handed on)."""
    fill = fill if fill is not None else filling_sequence
    side = int(round(len(tokens_list) ** 0.5))
    assert side == 32 and side * side == len(tokens_list)
    code = tokens_list.view(side, side)
    midfix = torch.tensor([tokenizer[m] for m in ('[EOI1]', '[ROI2]', '[POS0]', '[BASE]', '[BOI2]')], device=code.device)
    big = torch.full((2 * side, 2 * side), -1, dtype=torch.long, device=code.device)
    only_image_codes = [slice(tokenizer.img_tokenizer.num_tokens, None)]
    for bi, bj, lines in _MAGNIFY_WINDOWS:
        patch = code[8 * bi: 8 * (bi + 2), 8 * bj: 8 * (bj + 2)].reshape(-1)
        target = big[16 * bi: 16 * bi + lines, 16 * bj: 16 * (bj + 2)]
        context = torch.cat([text_token_list, patch, midfix], dim=0)
        done = fill(model, torch.cat([context, target.reshape(-1)], dim=0), args, invalid_slices=only_image_codes, tokenizer=tokenizer)
        big[16 * bi: 16 * bi + lines, 16 * bj: 16 * (bj + 2)] = done[0, len(context):].view(lines, 32)
    return big.view(1, 4 * side * side)


def _markers(tokenizer):
    n_img, n_txt = tokenizer.img_tokenizer.num_tokens, tokenizer.txt_tokenizer.num_tokens
    boi, eoi = (tokenizer['[BOI1]'], tokenizer['[BOI2]']), (tokenizer['[EOI1]'], tokenizer['[EOI2]'])
    return n_img, n_txt, boi, eoi, tokenizer['[ROI2]']


def _plan_context(seq_l, tokenizer):
    """The context walk of the device planners (filling_sequence's, up to its first model call): the given ids before the
    first mark, the slices the marker rule forbids after them, and the [ROI2] offset.  Returns (n, offset, invalid)."""
    n_img, n_txt, boi, eoi, roi2 = _markers(tokenizer)
    n, offset, invalid = 0, 100000, [slice(0, n_img)]
    while n < len(seq_l) and seq_l[n] >= 0:
        invalid = _slices_after(seq_l[n], invalid, n_img, n_txt, boi, eoi)
        if seq_l[n] == roi2:
            offset = n
        n += 1
    if n == 0:
        raise ValueError("the sequence must start with at least one given id")
    if n == len(seq_l):
        raise ValueError("nothing to generate: the sequence has no -1 / -nb marks")
    return n, offset, invalid


def _plan_allow(invalid, vocab):
    """The ids `invalid` leaves drawable, as the sampler's one (lo, hi) range."""
    kept, at = [], 0                                   # interval arithmetic on the host: a planner allocates no tensor
    for lo, hi, step in sorted(sl.indices(vocab) for sl in invalid):
        assert step == 1
        if lo >= hi:
            continue
        if lo > at:
            kept.append((at, lo))
        at = max(at, hi)
    if at < vocab:
        kept.append((at, vocab))
    if len(kept) != 1:
        raise NotImplementedError("the drawable ids are not one contiguous range: use filling_sequence")
    return kept[0]


def _plan_capacity(length):
    capacity = -(-length // 64) * 64
    if capacity > 4096:
        raise NotImplementedError(f"{length} positions exceed the decode cache's 4096 slots: use filling_sequence")
    return capacity


def plan_device_generation(seq_l, tokenizer, vocab):
    """Host planning of generate_on_device for a token list `seq_l` (filling_sequence's marks): a context of given ids, then
    ONE run of equal marks (-nb / -1).  Returns dict(context, run, nb, allow=(lo, hi), offset, capacity); `allow` is the range
    filling_sequence leaves drawable (its invalid slices after the context, by the same marker rule).  Raises
    NotImplementedError for what only filling_sequence does."""
    n, offset, invalid = _plan_context(seq_l, tokenizer)
    run = seq_l[n:]
    if any(t >= 0 for t in run):
        raise NotImplementedError("given ids after generated ones (beams shrink there): use filling_sequence")
    if any(t != run[0] for t in run):
        raise NotImplementedError("the beam count changes inside the run: use filling_sequence")
    allow = _plan_allow(invalid, vocab)
    return dict(context=n, run=len(run), nb=-run[0], allow=allow, offset=offset, capacity=_plan_capacity(len(seq_l)))


def plan_device_batch(seqs_l, tokenizer, vocab):
    """Host planning of generate_batch_on_device / DeviceGenerator for G token lists: plan_device_generation per sequence; the
    contexts may differ in length, but every sequence must have the same run length, the same nb and the same drawable
    range (one decode graph draws for all of them) -- otherwise NotImplementedError naming generate_on_device, which takes
    them one after another.  The [ROI2] offset may differ: it is applied to each prompt's position ids.
    Returns dict(contexts, pads, P, run, nb, rows, allow, offsets, capacity): P = the longest context, pads[g] = P - contexts[g]
    padding slots in front of prompt g (right-aligned contexts), rows = G * nb cache rows, capacity for P + run slots."""
    if not seqs_l:
        raise ValueError("no sequences")
    longest = max(len(seq_l) for seq_l in seqs_l)
    if longest > 4096:
        raise NotImplementedError(f"{longest} positions exceed the decode cache's 4096 slots (generate_on_device has the same limit): "
                                  f"use filling_sequence")
    plans = [plan_device_generation(list(seq_l), tokenizer, vocab) for seq_l in seqs_l]
    for what in ("run", "nb", "allow"):
        if any(p[what] != plans[0][what] for p in plans):
            raise NotImplementedError(f"the sequences differ in `{what}` ({[p[what] for p in plans]}): one decode graph draws the same "
                                      f"run for every row -- use generate_on_device per sequence")
    contexts = [p["context"] for p in plans]
    P, run, nb = max(contexts), plans[0]["run"], plans[0]["nb"]
    return dict(contexts=contexts, pads=[P - n for n in contexts], P=P, run=run, nb=nb, rows=len(plans) * nb, allow=plans[0]["allow"],
                offsets=[p["offset"] for p in plans], capacity=_plan_capacity(P + run))


def plan_device_fill(seq_l, tokenizer, vocab):
    """Host planning of DeviceFiller: what filling_sequence does with nb = 1 -- a context of given ids, then -1 marks with
    given ids anywhere after them (magnify's windows: lines an earlier window wrote sit between generated ones).
    Returns dict(context, given, replays, trailing, allow=(lo, hi), offset, capacity):
      given     one entry per position of seq_l: the id a decode step feeds there instead of drawing, -1 elsewhere (the
                context included: the prefill reads it);
      replays   decode steps after the prefill's first draw: one per position from context + 1 to the last mark;
      trailing  given ids after the last mark (copied on the host: no model call reads them).
    Raises NotImplementedError (naming filling_sequence) for -nb marks with nb > 1, a given [BOI*] / [EOI*] inside the run
    that changes the drawable range, [ROI2] inside the run, more than 4096 positions."""
    _, _, boi, eoi, roi2 = _markers(tokenizer)
    n_img, n_txt = tokenizer.img_tokenizer.num_tokens, tokenizer.txt_tokenizer.num_tokens
    n, offset, invalid = _plan_context(seq_l, tokenizer)
    marks = [i for i in range(n, len(seq_l)) if seq_l[i] < 0]
    if any(seq_l[i] != -1 for i in marks):
        raise NotImplementedError("-nb marks with nb > 1 (beams shrink at every given id): use filling_sequence")
    last = marks[-1]
    given = [-1] * len(seq_l)
    for i in range(n + 1, last):
        t = seq_l[i]
        if t < 0:
            continue
        if t == roi2:
            raise NotImplementedError("[ROI2] inside the run (positions restart there): use filling_sequence")
        if _slices_after(t, invalid, n_img, n_txt, boi, eoi) != invalid:
            raise NotImplementedError(f"given id {t} inside the run changes the drawable range: use filling_sequence")
        given[i] = t
    allow = _plan_allow(invalid, vocab)
    return dict(context=n, given=given, replays=last - n, trailing=len(seq_l) - 1 - last, allow=allow, offset=offset,
                capacity=_plan_capacity(len(seq_l)))


def plan_chunk_steps(given, context, replays, C):
    """The `replays` decode steps of a DeviceFiller call (plan_device_fill's given / context / replays) as model calls of width 1
    or C, for a decoder with a chunk step of C tokens (GraphDecoder(chunk=C)).  Step k of the plain run feeds the id of sequence
    position context + k.  Greedy from the first replay: at input position i a chunk of C is taken when the C - 1 positions after
    it are all given (they are fed from the table, nothing is drawn for them) and the chunk ends inside the run,
    i + C <= context + replays; otherwise one step.  Returns the list of widths; they sum to `replays`.  C = 0 or 1: all ones."""
    widths, i, end = [], context, context + replays
    while i < end:
        w = C if C > 1 and i + C <= end and all(t >= 0 for t in given[i + 1:i + C]) else 1
        widths.append(w)
        i += w
    return widths


def plan_device_batch_fill(seqs_l, tokenizer, vocab):
    """Host planning of DeviceBatchFiller for G token lists: plan_device_fill per sequence.  The contexts may differ in length
    (they are right-aligned, as plan_device_batch's), but counted from its own first mark every sequence must have the same
    `replays`, the same given positions inside the run and the same drawable range: one decode graph takes the same step --
    feed or draw, one token or a chunk -- for every row.  The nine magnify windows of different images are so by construction.
    Otherwise NotImplementedError naming DeviceFiller, which takes the sequences one after another.  The given IDS differ from
    row to row (cogv_sample_desc.given_stride); the [ROI2] offset may differ too.
    Returns dict(contexts, pads, P, replays, run = replays + 1, nb = 1, rows = G, allow, offsets, trailing, capacity, given,
    pattern): P / pads as plan_device_batch's; capacity for P + replays + 1 slots; given[g] the table of row g BY SLOT, capacity
    long -- given[g][pads[g] + i] = the entry of sequence position i in plan_device_fill's table, -1 elsewhere; pattern: the
    shared table by slot (0 where every row is given an id, -1 elsewhere) -- plan_chunk_steps(pattern, P, replays, C) are the
    widths of the run; trailing[g]: the given ids of sequence g after its last mark."""
    if not seqs_l:
        raise ValueError("no sequences")
    plans = [plan_device_fill(list(seq_l), tokenizer, vocab) for seq_l in seqs_l]
    inside = [[i - p["context"] for i, t in enumerate(p["given"]) if t >= 0] for p in plans]
    for what, values in (("`replays`", [p["replays"] for p in plans]), ("the given positions inside the run", inside),
                         ("`allow`", [p["allow"] for p in plans])):
        if any(v != values[0] for v in values):
            raise NotImplementedError(f"the sequences differ in {what}: one decode graph feeds or draws at the same step, from the same "
                                      f"range, for every row -- use DeviceFiller per sequence")
    contexts = [p["context"] for p in plans]
    P, replays = max(contexts), plans[0]["replays"]
    pads = [P - n for n in contexts]
    capacity = _plan_capacity(P + replays + 1)
    given = [[-1] * capacity for _ in plans]
    for row, p, pad in zip(given, plans, pads):
        n = p["context"]
        row[pad + n:pad + n + replays + 1] = p["given"][n:n + replays + 1]
    pattern = [-1] * capacity
    for k in inside[0]:
        pattern[P + k] = 0
    return dict(contexts=contexts, pads=pads, P=P, replays=replays, run=replays + 1, nb=1, rows=len(plans), allow=plans[0]["allow"],
                offsets=[p["offset"] for p in plans], trailing=[p["trailing"] for p in plans], capacity=capacity, given=given,
                pattern=pattern)


class _DeviceRun:
    """What the device entry points share: the refusals, ONE lazily built SamplingDecoder with its format keywords, the sampler
    armed for (temperature, top_k, top_p, allow) -- baked into a capture, so other values re-arm it and drop the graph, while the
    generator offset keeps counting -- and the run itself: start, capture once, generate.  generate_on_device and
    generate_batch_on_device use one for one call; DeviceGenerator, DeviceFiller and DeviceBatchFiller keep theirs call after call.
    .out [batch, width] receives the id drawn for sequence position out_base + j in column j; .given (DeviceFiller: [capacity],
    DeviceBatchFiller: [rows, capacity]) is the sampler's given table.  batch: the decoder's rows where the caller knows them
    before the first call (the refusal rule then also judges chunk= and weights= at that row count).  wide: SamplingDecoder's
    opt-in keyword (quantized weights at 9 ... 64 rows), handed on only where it is set.  kv_chunk: SamplingDecoder's opt-in keyword
    (opt-in; a later change makes it the default: chunk=C together with kv=), handed on only where it is set."""
    given = None

    def __init__(self, model, args, seed=0, capture=True, weights=None, kv=None, ragged=False, chunk=0, batch=None, wide=False,
                 kv_chunk=False):
        more = {}
        if wide:
            more["wide"] = True
        if kv_chunk:
            more["kv_chunk"] = True
        decoder.refuse_unsupported(weights, kv, ragged, args=args, model=model, use="filling_sequence", chunk=chunk, batch=batch, **more)
        self.model, self.seed, self.capture, self.ragged, self.chunk = model, int(seed), capture, ragged, int(chunk)
        self.formats = {"weights": weights}           # only the keywords that are set: a default build issues the call it always did
        if kv is not None:
            self.formats["kv"] = kv
        if ragged:
            self.formats["ragged"] = True
        if chunk:
            self.formats["chunk"] = self.chunk
        if wide:
            self.formats["wide"] = True
        if kv_chunk:
            self.formats["kv_chunk"] = True
        self.dec, self.key, self.out = None, None, None

    def size(self, batch, capacity, width=None, out_base=0):
        if not 0 < capacity <= 4096:
            raise ValueError(f"capacity {capacity} outside (0, 4096]: the decode cache's limit")
        self.batch, self.capacity, self.out_base = int(batch), int(capacity), out_base
        self.width = width if width is not None else self.capacity

    def vocab(self):
        return decoder.unwrap(self.model).word_embeddings.weight.shape[0]

    def _buffers(self, dev):
        self.out = torch.empty((self.batch, self.width), dtype=torch.long, device=dev)

    def arm(self, args, allow):
        """The decoder, built at the first call, with the sampler armed for this call's values."""
        if self.dec is None:
            self.dec = decoder.SamplingDecoder(self.model, batch=self.batch, capacity=self.capacity, **self.formats)
            self._buffers(self.dec.tok.device)
        key = (float(args.temperature), int(args.top_k), float(args.top_p), tuple(allow))
        if key != self.key:
            offset = self.dec.offset.clone() if self.key is not None else None
            self.dec.enable_sampling(*key[:3], allow=allow, seed=self.seed, out_tokens=self.out, out_base=self.out_base, given=self.given)
            if offset is not None:
                self.dec.offset.copy_(offset)
            self.dec.graph, self.key = None, key
            if self.chunk:
                self.dec.graph_chunk = None
        return self.dec

    def run(self, steps, *context, widths=None):
        """start / start_ragged on `context`, then `steps` decode steps on the graph (captured now unless an earlier call did).
        widths (a run driver with chunk=C): the steps as model calls of width 1 or C (plan_chunk_steps)."""
        dec = self.dec
        with torch.no_grad():
            (dec.start_ragged if self.ragged else dec.start)(*context)
            if steps:
                if self.capture and dec.graph is None:
                    dec.capture()
                if widths is None:
                    dec.generate(steps)
                else:
                    dec.generate(steps, widths=widths)
        return dec.scores.clone()


def generate_on_device(model, seq, args, tokenizer=None, seed=0, capture=True, weights=None, kv=None, wide=False):
    """filling_sequence for one run of generated tokens with the sampling on the device: prefill of the context (one row,
    its keys / values broadcast into the nb cache rows), nb independent first draws from its last logits, then one
    captured decode graph per token (generation/decoder.py SamplingDecoder) whose last launch filters, draws, and feeds
    the drawn id to the next replay.  Same filter as filling_sequence (temperature, invalid slices, top_k_logits; top_p per
    row); the draws come from the package's counter-based generator keyed (seed, step, row), not torch.multinomial.
    Supported: dense attention (args.is_sparse == 0), one model-parallel partition, fp16 / bf16, <= 4096 positions.
    Returns (tokens [nb, len(seq)], scores [nb] fp32: the summed log-probabilities of the drawn ids), on seq's device.
    capture=False runs the same launches eagerly (the reference for the captured form).
    weights="e4m3" | "mxfp4": the decode steps stream 8-bit or 4-bit copies of the weights (GraphDecoder's `weights`; the prefill
    stays 16-bit).
    kv="e4m3": the key/value caches hold 8-bit keys and values (GraphDecoder's `kv`); composes with `weights`.
    wide=True (opt-in; a later change makes it the default): with `weights` set, nb = 9 ... 64 rows run on the wide products of the
    quantized copies (GraphDecoder's `wide`) instead of being refused; no effect with 16-bit weights or up to 8 rows."""
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    drv = _DeviceRun(model, args, seed, capture, weights, kv, wide=wide)
    assert seq.dim() == 1
    plan = plan_device_generation(seq.tolist(), tokenizer, drv.vocab())
    n, run, nb = plan["context"], plan["run"], plan["nb"]
    tokens, attention_mask, position_ids = get_batch(seq[:n], seq.device, args)
    position_ids[position_ids > plan["offset"]] -= plan["offset"]
    drv.size(nb, plan["capacity"], width=run, out_base=n)
    drv.arm(args, plan["allow"])
    scores = drv.run(run - 1, tokens, position_ids, attention_mask)
    return torch.cat((tokens.expand(nb, n), drv.out), dim=1).to(seq.device), scores


def _batch_inputs(seqs, plan, device):
    """The right-aligned context block of a prompt set: tokens / position_ids [G, P] (padding columns zero: the ragged prefill
    fills them), each prompt's positions counted from 0 with its own [ROI2] offset applied."""
    G, P = len(seqs), plan["P"]
    tokens = torch.zeros((G, P), dtype=torch.long, device=device)
    position_ids = torch.zeros((G, P), dtype=torch.long, device=device)
    for g, (seq, n, pad, offset) in enumerate(zip(seqs, plan["contexts"], plan["pads"], plan["offsets"])):
        tokens[g, pad:] = seq[:n].to(device)
        pos = torch.arange(n, dtype=torch.long, device=device)
        pos[pos > offset] -= offset
        position_ids[g, pad:] = pos
    return tokens, position_ids


def _batch_run(drv, seqs, plan, args):
    """One prompt set through a ragged run driver.  Returns (per prompt [nb, len(seq_g)]: its context followed by the run its nb
    rows drew, scores [G, nb]); row g * nb + j is candidate j of prompt g."""
    P, run, nb = plan["P"], plan["run"], plan["nb"]
    dec = drv.arm(args, plan["allow"])
    tokens, position_ids = _batch_inputs(seqs, plan, dec.tok.device)
    scores = drv.run(run - 1, tokens, position_ids, plan["pads"])
    col0 = P - drv.out_base
    res = []
    for g, (seq, n) in enumerate(zip(seqs, plan["contexts"])):
        drawn = drv.out[g * nb:(g + 1) * nb, col0:col0 + run].to(seq.device)
        res.append(torch.cat((seq[:n].unsqueeze(0).expand(nb, n), drawn), dim=1))
    return res, scores.view(len(seqs), nb).to(seqs[0].device)


def generate_batch_on_device(model, seqs, args, tokenizer=None, seed=0, capture=True, weights=None, kv=None, wide=False):
    """generate_on_device for G prompts at once on ONE decode graph (the reference's generate_images_continually walks a file
    of prompts one after another, generate_samples.py:202-221; a decode step is a weight stream that costs little more for
    eight rows than for one).  seqs: list of 1-D tensors, each a context of given ids followed by one run of equal marks; the
    contexts may differ in length, the runs, nb and the drawable range may not (plan_device_batch).  The contexts are
    right-aligned in the caches (SamplingDecoder(ragged=True)): one prefill under a per-prompt mask, then every replay draws
    one token for all G * nb rows -- row g * nb + j is candidate j of prompt g.
    Returns (list of G tensors [nb, len(seq_g)] without padding, scores [G, nb] fp32), on the sequences' device.
    One prompt is generate_on_device itself (the plain decoder: same launches, same bits).  weights / kv / capture / seed / wide
    (opt-in: quantized weights at 9 ... 64 rows; a later change makes it the default) as there."""
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    seqs = list(seqs)
    assert seqs and all(seq.dim() == 1 for seq in seqs)
    if len(seqs) == 1:
        more = {"wide": True} if wide else {}
        tokens, scores = generate_on_device(model, seqs[0], args, tokenizer=tokenizer, seed=seed, capture=capture, weights=weights, kv=kv, **more)
        return [tokens], scores.view(1, -1)
    drv = _DeviceRun(model, args, seed, capture, weights, kv, ragged=True, wide=wide)
    plan = plan_device_batch([seq.tolist() for seq in seqs], tokenizer, drv.vocab())
    drv.size(plan["rows"], plan["capacity"], width=plan["run"], out_base=plan["P"])
    return _batch_run(drv, seqs, plan, args)


class DeviceGenerator(_DeviceRun):
    """generate_batch_on_device on ONE ragged SamplingDecoder and ONE captured decode graph that are reused call after call --
    DeviceFiller's counterpart for a file of prompts (generate_samples.py:202-221): `gen = DeviceGenerator(model, args, rows=8);
    tokens, scores = gen(seqs)` for any prompt set with G * nb == rows and P + run <= capacity.  What changes from call to call
    is device data: the caches, `first`, the token / position / slot buffers, the generator offset (it keeps counting across
    calls, so every call draws fresh numbers) and the output buffer ([rows, capacity], column = slot).  Temperature, top-k /
    top-p and the drawable range are baked into the capture: a call with other values re-arms the sampler and captures again.
    A single prompt (G = 1) runs on the same ragged decoder with first = 0.  capture / weights / kv / wide as generate_on_device's
    (wide=True: opt-in, quantized weights at 9 ... 64 rows; a later change makes it the default)."""

    def __init__(self, model, args, rows, capacity=1152, seed=0, capture=True, weights=None, kv=None, wide=False):
        super().__init__(model, args, seed, capture, weights, kv, ragged=True, wide=wide)
        self.size(rows, capacity)
        if rows < 1:
            raise ValueError(f"rows = {rows} must be positive")
        self.rows, self.args = self.batch, args

    def _buffers(self, dev):
        self.out = torch.zeros((self.rows, self.capacity), dtype=torch.long, device=dev)

    def __call__(self, seqs, args=None, tokenizer=None):
        """seqs: list of 1-D tensors (generate_batch_on_device's); args: the sampling arguments of this call (default: the
        constructor's).  Returns (list of [nb, len(seq_g)] token tensors, scores [G, nb] fp32)."""
        args = args if args is not None else self.args
        decoder.refuse_unsupported(args=args, use="filling_sequence")
        tokenizer = tokenizer if tokenizer is not None else IdSpace()
        seqs = list(seqs)
        assert seqs and all(seq.dim() == 1 for seq in seqs)
        plan = plan_device_batch([seq.tolist() for seq in seqs], tokenizer, self.vocab())
        if plan["rows"] != self.rows:
            raise ValueError(f"{len(seqs)} prompts x {plan['nb']} rows = {plan['rows']} rows: this generator was built for {self.rows}")
        if plan["P"] + plan["run"] > self.capacity:
            raise NotImplementedError(f"{plan['P'] + plan['run']} positions exceed this generator's {self.capacity} decode slots: use "
                                      f"generate_on_device or a larger capacity")
        return _batch_run(self, seqs, plan, args)


class DeviceFiller(_DeviceRun):
    """filling_sequence for nb = 1 on ONE captured decode graph that is reused call after call: magnify's sequence filler
    (`magnify(model, tokenizer, code, text, args, fill=DeviceFiller(model, args))`, super-resolution).  Per call: the given
    table goes to the device, the context is prefilled (one eager model call) and its last logits draw the first mark, then
    one graph replay per later position up to the last mark -- the sampler inside it draws at a mark and feeds the given
    id elsewhere (cogv_sample_desc.given); given ids after the last mark are copied on the host.
    What changes from call to call is device data: the given table, the token / position / slot buffers, the generator
    offset (it keeps counting across calls, so every window draws fresh numbers) and the output row ([1, capacity],
    column = sequence position).  Temperature, top-k / top-p and the drawable range are baked into the capture: a call
    with other values re-arms the sampler and captures again.
    Same filter as filling_sequence; draws from the package's counter-based generator keyed (seed, step, row).  Dense
    attention, one model-parallel partition, <= capacity positions (1408: the reference's MAXSEQLEN 1345 rounded up to 64).
    capture=False runs the same launches eagerly.  After a call, .scores is [1] fp32: the summed log-probability of the
    drawn ids (given ids add nothing).  weights="e4m3": the decode steps stream 8-bit copies of the weights (GraphDecoder's
    `weights`), made when the first call builds the decoder.  kv="e4m3": 8-bit key/value caches (GraphDecoder's `kv`).
    chunk=C (2 ... 8; GraphDecoder's `chunk`, 16-bit cache only): runs of given ids inside the run are fed as chunk steps of C
    tokens -- one model call in place of C replays, planned per call by plan_chunk_steps; a second graph is captured next to
    the one-token one.  The draws keep their generator counters (one per position), but a chunk step's logits differ in the last
    bits from one-token steps' (the Sandwich-LN scale spans the chunk's rows), so a draw can differ from the chunk=0 filler's
    where two ids are about equally likely.  .model_calls: the decode steps of the last call.  0 (default): nothing changes.
    kv_chunk=True (opt-in; a later change makes it the default): chunk=C together with kv="e4m3" is accepted -- the chunk steps run
    on the 8-bit cache (GraphDecoder's `kv_chunk`, ops.attention_decode_chunk_kv8).  With kv=None or chunk=0 it does
    nothing; False: the pair is refused as it always was."""

    def __init__(self, model, args, seed=0, capacity=1408, capture=True, weights=None, kv=None, chunk=0, kv_chunk=False):
        more = {"kv_chunk": True} if kv_chunk else {}
        super().__init__(model, args, seed, capture, weights, kv, chunk=chunk, **more)
        self.size(1, capacity)
        self.scores = None
        self.model_calls = 0

    def _buffers(self, dev):
        super()._buffers(dev)
        self.given = torch.full((self.capacity,), -1, dtype=torch.long, device=dev)

    def __call__(self, model, seq, args, invalid_slices=None, tokenizer=None):
        """filling_sequence's signature and result: the completed row [1, len(seq)] on seq's device.  invalid_slices is
        ignored in favour of the marker rule, as filling_sequence ignores it."""
        decoder.refuse_unsupported(args=args, use="filling_sequence")
        if model is not self.model:
            raise ValueError("this DeviceFiller was built for another model")
        assert seq.dim() == 1
        if len(seq) > self.capacity:
            raise NotImplementedError(f"{len(seq)} positions exceed this filler's {self.capacity} decode slots: use "
                                      f"filling_sequence or a larger capacity")
        tokenizer = tokenizer if tokenizer is not None else IdSpace()
        seq_l = seq.tolist()
        plan = plan_device_fill(seq_l, tokenizer, self.vocab())
        n, replays = plan["context"], plan["replays"]
        dec = self.arm(args, plan["allow"])
        tokens, attention_mask, position_ids = get_batch(seq[:n], dec.tok.device, args)
        position_ids[position_ids > plan["offset"]] -= plan["offset"]
        table = torch.full((self.capacity,), -1, dtype=torch.long)
        table[:len(seq_l)] = torch.tensor(plan["given"], dtype=torch.long)
        self.given.copy_(table)                       # before start(): its draw reads the entry of position n (-1)
        if self.chunk:
            widths = plan_chunk_steps(plan["given"], n, replays, self.chunk)
            self.model_calls = len(widths)
            self.scores = self.run(replays, tokens, position_ids, attention_mask, widths=widths)
        else:
            self.model_calls = replays
            self.scores = self.run(replays, tokens, position_ids, attention_mask)
        out = seq.clone()
        out[n:n + replays + 1] = self.out[0, n:n + replays + 1].to(seq.device)
        return out.unsqueeze(0)


class DeviceBatchFiller(_DeviceRun):
    """DeviceFiller for several sequences at once on ONE ragged SamplingDecoder and ONE captured decode graph that are reused
    call after call: the same window of several images (magnify_batch: `fill=DeviceBatchFiller(model, args, rows=G)`), as
    DeviceGenerator is generate_on_device for several prompts.  A decode step is a weight stream, so `rows` images cost little
    more per step than one.  `filler(seqs)` takes 1 <= G <= rows sequences that plan_device_batch_fill accepts (contexts of any
    lengths, right-aligned in the caches; the same marks and given positions counted from each first mark, with every row's OWN
    given ids); spare rows repeat the last sequence and are dropped from the result.  Per call: every row's given table goes to
    the device by slot ([rows, capacity]; the sampler reads row r's at r * given_stride), one ragged prefill draws every row's
    first mark, then one replay per later slot up to the last mark -- each row is fed or draws on its own.  The output buffer is
    [rows, capacity] with column = slot.  Returns the list of G completed rows [1, len(seq_g)] on each sequence's device; given
    ids after the last mark are kept from the input.  After a call .scores is [G] fp32 and .model_calls the decode steps, as
    DeviceFiller's.  Temperature, top-k / top-p and the drawable range are baked into the capture (a call with other values
    re-arms and captures again); the generator offset keeps counting across calls.
    capture / weights / kv as DeviceFiller's.  chunk=C: runs of given ids are fed as chunk steps on a second graph (rows * C <= 8
    rows per step; 16-bit cache only, unless kv_chunk=True -- opt-in; a later change makes it the default: the chunk steps then run on
    the 8-bit cache of kv="e4m3", GraphDecoder's `kv_chunk`).  Above 8 rows the decoder takes the wide step (9 ... 24 rows) or the tile kernels by
    itself; weights="e4m3" covers up to 8 rows, so it is refused above them -- unless wide=True (opt-in; a later change makes it
    the default): 9 ... 64 rows then run on the wide products of the quantized copies (GraphDecoder's `wide`: 1.05-1.17x the 16-bit
    wide step's speed at 12 ... 64 rows of the captured 4B step, not faster than the tile kernels from 48 rows on).  Dense attention, one model-parallel partition, fp16 / bf16, P + replays + 1 <= capacity
    slots."""

    def __init__(self, model, args, rows, capacity=1408, seed=0, capture=True, weights=None, kv=None, chunk=0, wide=False,
                 kv_chunk=False):
        more = {"kv_chunk": True} if kv_chunk else {}
        super().__init__(model, args, seed, capture, weights, kv, ragged=True, chunk=chunk, batch=rows, wide=wide, **more)
        if rows < 1:
            raise ValueError(f"rows = {rows} must be positive")
        self.size(rows, capacity)
        self.rows, self.args = self.batch, args
        self.scores = None
        self.model_calls = 0

    def _buffers(self, dev):
        self.out = torch.zeros((self.rows, self.capacity), dtype=torch.long, device=dev)
        self.given = torch.full((self.rows, self.capacity), -1, dtype=torch.long, device=dev)

    def __call__(self, seqs, args=None, tokenizer=None):
        """seqs: list of 1-D tensors (filling_sequence's marks, nb = 1); args: the sampling arguments of this call (default: the
        constructor's).  Returns the list of completed rows [1, len(seq_g)]."""
        args = args if args is not None else self.args
        decoder.refuse_unsupported(args=args, use="filling_sequence")
        tokenizer = tokenizer if tokenizer is not None else IdSpace()
        seqs = list(seqs)
        if not 1 <= len(seqs) <= self.rows:
            raise ValueError(f"{len(seqs)} sequences: this filler was built for 1 ... {self.rows}")
        assert all(seq.dim() == 1 for seq in seqs)
        G = len(seqs)
        filled = seqs + [seqs[-1]] * (self.rows - G)                      # spare rows repeat the last sequence
        plan = plan_device_batch_fill([seq.tolist() for seq in filled], tokenizer, self.vocab())
        P, replays = plan["P"], plan["replays"]
        if P + replays + 1 > self.capacity:
            raise NotImplementedError(f"{P + replays + 1} slots exceed this filler's {self.capacity} decode slots: use DeviceFiller "
                                      f"per sequence or a larger capacity")
        dec = self.arm(args, plan["allow"])
        tokens, position_ids = _batch_inputs(filled, plan, dec.tok.device)
        width = min(plan["capacity"], self.capacity)                      # (entries past P + replays are -1)
        table = torch.full((self.rows, self.capacity), -1, dtype=torch.long)
        table[:, :width] = torch.tensor(plan["given"], dtype=torch.long)[:, :width]
        self.given.copy_(table)                       # before start_ragged(): its draw reads the entries of slot P (-1)
        if self.chunk:
            widths = plan_chunk_steps(plan["pattern"], P, replays, self.chunk)
            self.model_calls = len(widths)
            scores = self.run(replays, tokens, position_ids, plan["pads"], widths=widths)
        else:
            self.model_calls = replays
            scores = self.run(replays, tokens, position_ids, plan["pads"])
        self.scores = scores[:G].to(seqs[0].device)
        res = []
        for g, (seq, n) in enumerate(zip(seqs, plan["contexts"])):
            out = seq.clone()
            out[n:n + replays + 1] = self.out[g, P:P + replays + 1].to(seq.device)
            res.append(out.unsqueeze(0))
        return res


def magnify_batch(model, tokenizer, codes, texts, args, fill=None):
    """magnify for G images at once (the reference's super-resolution task walks a file of images one after another,
    generate_samples.py generate_images_continually; post-selection keeps several candidates per prompt).  codes: [G, 1024] or a
    list of G 1-D tensors of 1024 codes; texts: list of G 1-D tensors of any lengths.  The nine windows run in magnify's order;
    window w of ALL images is one call `fill(seqs, args, tokenizer=tokenizer)` with the G window sequences, which returns the
    list of G completed rows [1, len(seq_g)] -- DeviceBatchFiller(model, args, rows=G) does it on one decode graph (the windows
    of different images differ in their ids, not in where the marks are).  Default `fill`: filling_sequence per sequence.
    Returns [G, 4096] codes."""
    if fill is None:
        def fill(seqs, args_, tokenizer=None):
            return [filling_sequence(model, seq, args_, tokenizer=tokenizer) for seq in seqs]
    codes = list(codes)
    G = len(codes)
    if len(texts) != G:
        raise ValueError(f"{G} code maps but {len(texts)} texts")
    maps = [code.view(32, 32) for code in codes]
    dev = maps[0].device
    midfix = torch.tensor([tokenizer[m] for m in ('[EOI1]', '[ROI2]', '[POS0]', '[BASE]', '[BOI2]')], device=dev)
    big = torch.full((G, 64, 64), -1, dtype=torch.long, device=dev)
    for bi, bj, lines in _MAGNIFY_WINDOWS:
        contexts = [torch.cat([text.to(dev), m[8 * bi: 8 * (bi + 2), 8 * bj: 8 * (bj + 2)].reshape(-1), midfix], dim=0)
                    for text, m in zip(texts, maps)]
        seqs = [torch.cat([context, big[g, 16 * bi: 16 * bi + lines, 16 * bj: 16 * (bj + 2)].reshape(-1)], dim=0)
                for g, context in enumerate(contexts)]
        done = fill(seqs, args, tokenizer=tokenizer)
        for g, (context, row) in enumerate(zip(contexts, done)):
            big[g, 16 * bi: 16 * bi + lines, 16 * bj: 16 * (bj + 2)] = row[0, len(context):].view(lines, 32)
    return big.view(G, 4096)
