"""GPU: the decode step of C tokens per cache row at the model level -- GraphDecoder(chunk=C).step_chunk against the
full-sequence forward (chain at 4 rows, layer by layer at 8; eager and captured; 16-bit and 8-bit weights), the one-token step on
the cache a chunk step wrote, chunk steps inside a sampling run (SamplingDecoder.generate(n, widths=...)) and
DeviceFiller(chunk=8) under the checks of tests/test_device_fill_gpu.py."""
import pytest
import torch

from cogview_amd.generation import DeviceFiller, GraphDecoder, SamplingDecoder, plan_chunk_steps, plan_device_fill
from tests.generation_cases import COIN_FLIP
from tests.test_device_fill_gpu import _args, _check_generated_at_argmax, _teacher_forced_gaps, _toy, _window
from tests.test_w8_decode_gpu import TOL, rel

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
L_, V_, H_, NH_, S_, PRE, CHUNKED = 3, 1024, 512, 8, 48, 23, 16         # 16 positions in chunk steps, then one-token steps
_MODELS, _FULL, _RUNS = {}, {}, {}


def _model(dtype):
    if dtype not in _MODELS:
        from cogview_amd.fp16 import FP16_Module
        from cogview_amd.model import GPT2Model
        torch.manual_seed(11)
        m = GPT2Model(L_, V_, H_, NH_, 0.0, 0.0, 0.0, S_ + 1, 64, False)
        for n, p in m.named_parameters():                      # non-trivial LayerNorm affine / biases
            if p.dim() == 1:
                p.data.add_(0.1 * torch.randn_like(p))
        _MODELS[dtype] = FP16_Module(m.cuda(), dtype=dtype, keep_half_outputs=True).eval()
    return _MODELS[dtype]


def _tokens(B, vocab=V_, n=S_):
    tokens = torch.randint(0, vocab, (B, n), generator=torch.Generator().manual_seed(3)).cuda()
    return tokens, torch.arange(n, device="cuda").unsqueeze(0).expand(B, -1)


def _full(dtype, B):
    """the full-sequence forward, computed once per (dtype, batch)"""
    if (dtype, B) not in _FULL:
        tokens, pos = _tokens(B)
        with torch.no_grad():
            _FULL[(dtype, B)] = model_logits = _model(dtype)(tokens, pos, 0, None, None, 0)[0]
        assert model_logits.shape == (B, S_, V_)
    return _FULL[(dtype, B)]


def _chunk_run(model, tokens, pos, pre, B, C, captured, steps_after=2, **kw):
    """prefill `pre` positions, CHUNKED positions in chunk steps of C, then one-token steps -> (decoder, logits [B, CHUNKED + after, V])"""
    dec = GraphDecoder(model, batch=B, capacity=128, chunk=C, **kw)
    dec.prefill(tokens[:, :pre], pos[:, :pre])
    if captured:
        dec.capture()
        assert dec.graph is not None and dec.graph_chunk is not None
    outs = []
    for t in range(pre, pre + CHUNKED, C):
        outs.append(dec.step_chunk(tokens[:, t:t + C], pos[:, t:t + C]).clone())
        assert outs[-1].shape[:2] == (B, C)
    for t in range(pre + CHUNKED, pre + CHUNKED + steps_after):
        outs.append(dec.step(tokens[:, t:t + 1], pos[:, t:t + 1]).clone())
    assert dec.length == pre + CHUNKED + steps_after
    return dec, torch.cat(outs, 1)


def _run(dtype, B, C, captured):
    key = (dtype, B, C, captured)
    if key not in _RUNS:
        _RUNS[key] = _chunk_run(_model(dtype), *_tokens(B), PRE, B, C, captured)[1]
    return _RUNS[key]


# 4 rows: the chain; 8 rows: layer by layer, as one cache row of 8 tokens and as two of 4
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", [(1, 4), (1, 8), (2, 4)])
def test_chunk_steps_match_the_full_sequence_forward(dtype, B, C):
    from cogview_amd import functional as F_
    tr = _model(dtype).module.transformer
    assert F_.decode_chain_supported(tr, 4) and not F_.decode_chain_supported(tr, 8)
    full = _full(dtype, B)
    for captured in (False, True):
        out = _run(dtype, B, C, captured)
        e_chunk = rel(out[:, :CHUNKED], full[:, PRE:PRE + CHUNKED])
        e_after = rel(out[:, CHUNKED:], full[:, PRE + CHUNKED:PRE + CHUNKED + 2])
        print(f"[{dtype}] batch {B} chunk {C} captured={captured}: chunk steps vs full sequence rel-L2 {e_chunk:.2e}, "
              f"one-token steps on the chunks' cache {e_after:.2e}")
        assert e_chunk < TOL[dtype] and e_after < TOL[dtype]
    assert torch.equal(_run(dtype, B, C, True), _run(dtype, B, C, False)), "graph replay must reproduce the eager chunk step bit for bit"


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_step_writes_the_cache_the_one_token_steps_write(dtype):
    """keys / values depend on the layer inputs, which differ in the last bits between the two steps (the Sandwich scale spans the
    chunk's rows), so they are held to the logits' bar; nothing is written past the chunk"""
    model = _model(dtype)
    tokens, pos = _tokens(1)
    dec, _ = _chunk_run(model, tokens, pos, PRE, 1, 4, False, steps_after=0)
    one = GraphDecoder(model, batch=1, capacity=128)
    one.prefill(tokens[:, :PRE], pos[:, :PRE])
    for t in range(PRE, PRE + CHUNKED):
        one.step(tokens[:, t:t + 1], pos[:, t:t + 1])
    n = PRE + CHUNKED
    for a, b in zip(dec.caches, one.caches):
        assert rel(a[:, :n], b[:, :n]) < TOL[dtype]
        assert torch.equal(a[:, n:], b[:, n:])                   # nothing written past the chunk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [4, 8])
def test_chunk_steps_on_8bit_weights_match_the_one_token_8bit_decoder(dtype, C):
    from tests import test_w8_decode_gpu as W8
    model = W8._model(dtype)
    tokens, pos = _tokens(1, vocab=W8.V_, n=64)
    pre = 30
    one = GraphDecoder(model, batch=1, capacity=128, weights="e4m3")
    one.prefill(tokens[:, :pre], pos[:, :pre])
    ref = torch.cat([one.step(tokens[:, t:t + 1], pos[:, t:t + 1]).clone() for t in range(pre, pre + CHUNKED + 2)], 1)
    res = {}
    for captured in (False, True):
        dec, res[captured] = _chunk_run(model, tokens, pos, pre, 1, C, captured, weights="e4m3")
        assert dec.w8 is not None
        e = rel(res[captured], ref)
        print(f"[{dtype}] chunk {C} captured={captured}: 8-bit chunk steps vs the 8-bit one-token decoder rel-L2 {e:.2e}")
        assert e < TOL[dtype]
    assert torch.equal(res[True], res[False])


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_steps_on_a_ragged_decoder_match_its_one_token_steps(dtype):
    """two prompts of 23 and 17 tokens right-aligned in one decoder (ragged=True): chunk steps of 4 per cache row against the
    one-token steps of the same decoder form, at the decode tests' bar"""
    model = _model(dtype)
    tokens, _ = _tokens(2)
    pads, P = [0, 6], PRE
    pos = torch.stack([torch.arange(S_, device="cuda") - p for p in pads]).clamp(min=0)          # each prompt counts from its own start
    res = {}
    for C in (0, 4):
        dec = GraphDecoder(model, batch=2, capacity=128, ragged=True, chunk=C)
        with torch.no_grad():
            dec._prefill(tokens[:, :P].clone(), pos[:, :P].clone(), None, pads)
        assert dec.first.tolist() == pads
        step = C or 1
        outs = []
        for t in range(P, P + CHUNKED, step):
            outs.append((dec.step_chunk if C else dec.step)(tokens[:, t:t + step], pos[:, t:t + step]).clone())
        res[C] = torch.cat(outs, 1)
    e = rel(res[4], res[0])
    print(f"[{dtype}] ragged, chunk 4 against one-token steps: rel-L2 {e:.2e}")
    assert torch.isfinite(res[4].float()).all() and e < TOL[dtype]


# ---------------------------------------------------------------------------------------------- chunk steps inside a sampling run
STATE = ("tok", "pos", "pos_index", "table", "offset", "out_tokens", "scores")


def _sampling_run(dtype, given_l, n, replays, C, captured, widths):
    model = _model(dtype)
    tokens, pos = _tokens(1)
    dec = SamplingDecoder(model, batch=1, capacity=64, chunk=C)
    given = torch.tensor(given_l + [-1] * (64 - len(given_l)), dtype=torch.long, device="cuda")
    out = torch.full((1, 64), -7, dtype=torch.long, device="cuda")
    dec.enable_sampling(temperature=1.02, top_k=50, seed=5, out_tokens=out, given=given)
    dec.start(tokens[:1, :n], pos[:1, :n])
    if captured:
        dec.capture()
    dec.generate(replays, widths=widths)
    torch.cuda.synchronize()
    return dec, {k: getattr(dec, k).clone() for k in STATE}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("captured", [False, True])
def test_a_run_of_given_ids_in_chunks_leaves_the_state_of_one_by_one(dtype, captured):
    n, replays = 10, 30
    g = torch.Generator().manual_seed(8)
    given_l = [-1] * n + torch.randint(0, V_, (replays + 1,), generator=g).tolist()         # positions n ... n + replays: all given
    _, plain = _sampling_run(dtype, given_l, n, replays, 0, captured, None)
    for C in (4, 8):
        widths = plan_chunk_steps(given_l, n, replays, C)
        assert widths == [C] * (replays // C) + [1] * (replays % C)
        dec, st = _sampling_run(dtype, given_l, n, replays, C, captured, widths)
        assert dec.chunk_steps == replays // C and dec.length == n + replays
        for k in STATE:
            assert torch.equal(st[k], plain[k]), (C, k)
    assert plain["out_tokens"][0, n:n + replays + 1].tolist() == given_l[n:] and int(plain["pos_index"]) == n + replays
    assert int(plain["offset"]) == replays + 1 and float(plain["scores"]) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_mixed_run_keeps_the_generator_offset_and_the_write_slot(dtype):
    n, replays = 10, 36                                            # positions 10 ... 46 of the model's 49
    given_l = [-1] * 64
    g = torch.Generator().manual_seed(9)
    for lo, hi in ((13, 22), (25, 28), (31, 47)):                  # runs of 9, 3 and 16 given ids between drawn ones
        given_l[lo:hi] = torch.randint(0, V_, (hi - lo,), generator=g).tolist()
    _, plain = _sampling_run(dtype, given_l, n, replays, 0, True, None)
    for C in (4, 8):
        widths = plan_chunk_steps(given_l, n, replays, C)
        dec, st = _sampling_run(dtype, given_l, n, replays, C, True, widths)
        assert dec.chunk_steps == sum(1 for w in widths if w > 1) > 0
        assert torch.equal(st["offset"], plain["offset"]) and torch.equal(st["pos_index"], plain["pos_index"])
        assert torch.equal(st["pos"], plain["pos"]) and torch.equal(st["table"], plain["table"])
        row, is_given = st["out_tokens"][0, n:n + replays + 1], torch.tensor(given_l[n:n + replays + 1]) >= 0
        assert row[is_given.cuda()].tolist() == [t for t in given_l[n:n + replays + 1] if t >= 0]
        assert int(row.min()) >= 0 and bool(torch.isfinite(st["scores"]).all()) and float(st["scores"]) < 0


# ------------------------------------------------------------------------------------------------------------ DeviceFiller(chunk=8)
LINES, GIVEN_LINES = 10, 7


def _fill(model, seq, ids, args, **kw):
    f = DeviceFiller(model, args, **kw)
    return f, f(model, seq.clone(), args, tokenizer=ids)[0]


def test_greedy_fill_in_chunks(golden_dir):
    z, c, ids, model = _toy(golden_dir)
    seq = _window(z, c, ids, lines=LINES, given_lines=GIVEN_LINES)
    plan = plan_device_fill(seq.tolist(), ids, int(z["vocab"]))
    f, out = _fill(model, seq, ids, _args(), chunk=8)
    widths = plan_chunk_steps(plan["given"], plan["context"], plan["replays"], 8)
    assert f.model_calls == len(widths) < plan["replays"] and f.dec.chunk_steps == sum(1 for w in widths if w > 1) == 2 * (GIVEN_LINES - 1)
    assert f.dec.graph is not None and f.dec.graph_chunk is not None
    _check_generated_at_argmax(model, seq, out, ids, c["img_tokens"])
    f0, ref = _fill(model, seq, ids, _args())
    assert f0.model_calls == plan["replays"]
    _, gap = _teacher_forced_gaps(model, out, ids, c["img_tokens"])
    diff = (out != ref).nonzero().flatten()
    if diff.numel():                                       # a first divergence from the chunk=0 filler only at a coin flip
        i = int(diff[0])
        assert gap[i] < COIN_FLIP, (i, float(gap[i]))


def test_captured_fill_in_chunks_equals_eager(golden_dir):
    z, c, ids, model = _toy(golden_dir)
    seq = _window(z, c, ids, lines=LINES, given_lines=GIVEN_LINES, seed=1)
    args = _args(top_k=200, temperature=1.02)
    res = []
    for cap in (True, False):
        f, out = _fill(model, seq, ids, args, seed=1234, capture=cap, chunk=8)
        res.append((out, f.scores))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    given = seq >= 0
    assert torch.equal(res[0][0][given], seq[given]) and int(res[0][0][~given].max()) < c["img_tokens"]
    assert torch.isfinite(res[0][1]).all() and float(res[0][1]) < 0


def test_reused_chunk_filler_equals_a_fresh_one(golden_dir):
    z, c, ids, model = _toy(golden_dir)
    long_seq = _window(z, c, ids, lines=LINES + 2, given_lines=0, seed=2)
    short_seq = _window(z, c, ids, lines=LINES, given_lines=GIVEN_LINES, seed=3)
    reused = DeviceFiller(model, _args(), chunk=8)
    reused(model, long_seq.clone(), _args(), tokenizer=ids)
    assert reused.dec.chunk_steps == 0
    a = reused(model, short_seq.clone(), _args(), tokenizer=ids)
    _, b = _fill(model, short_seq, ids, _args(), chunk=8)
    assert torch.equal(a[0], b)
