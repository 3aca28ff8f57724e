"""GPU: the chunk step on the 8-bit key/value cache at the model level -- GraphDecoder(chunk=C, kv="e4m3", kv_chunk=True), eager
and captured, with 16-bit, E4M3 and MXFP4 weights and on a ragged decoder, and the fillers that hand the keywords on.  The models
are those of tests/test_kv8_decode_gpu.py and tests/test_w4_decode_gpu.py (2 layers, h = 1024, 16 heads).  A prefill of 117 tokens,
16 positions in chunk steps (slots 117 ... 132: the run crosses the boundary between the first and the second 128-key split), then
two one-token steps.

The oracle comparison takes every layer's keys and values from the decoder's OWN cache (dequantize()), as
tests/test_kv8_decode_gpu.py does and for its reason; row j of a chunk step attends the slots up to its own, and the Sandwich-LN
scale is taken over the step's rows."""
import types

import pytest
import torch

from oracle import cogview_oracle as O
from cogview_amd.generation import DeviceFiller, GraphDecoder, plan_chunk_steps, plan_device_fill
from tests.generation_cases import ToyIds
from tests.test_kv8_decode_gpu import _args, _context, _model
from tests.test_w8_decode_gpu import L_, H_, NH_, N_IMG, N_TXT, V_, TOL, rel

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
CAP, PRE, CHUNKED, AFTER = 192, 117, 16, 2
N = PRE + CHUNKED + AFTER
SHAPES = [(1, 4), (1, 8), (2, 4)]          # 4 rows: the chain; 8 rows: layer by layer, as one cache row of 8 tokens and as two of 4


def _tokens(B, n=N):
    tokens = torch.randint(0, V_, (B, n), generator=torch.Generator().manual_seed(3)).cuda()
    return tokens, torch.arange(n, device="cuda").unsqueeze(0).expand(B, -1)


def _chunk_run(model, tokens, pos, pre, B, C, captured, capacity=CAP, **kw):
    """prefill `pre` positions, CHUNKED positions in chunk steps of C (C = 0: in one-token steps), then AFTER one-token steps
    -> (decoder, logits [B, CHUNKED + AFTER, V])"""
    dec = GraphDecoder(model, batch=B, capacity=capacity, chunk=C, **kw)
    dec.prefill(tokens[:, :pre], pos[:, :pre])
    if captured:
        dec.capture()
        assert dec.graph is not None and (not C or dec.graph_chunk is not None)
    outs = []
    if C:
        for t in range(pre, pre + CHUNKED, C):
            outs.append(dec.step_chunk(tokens[:, t:t + C], pos[:, t:t + C]).clone())
            assert outs[-1].shape[:2] == (B, C)
    for t in range(pre + (CHUNKED if C else 0), pre + CHUNKED + AFTER):
        outs.append(dec.step(tokens[:, t:t + 1], pos[:, t:t + 1]).clone())
    assert dec.length == pre + CHUNKED + AFTER
    return dec, torch.cat(outs, 1)


_RUNS = {}


def _run(dtype, B, C, captured, kv="e4m3"):
    key = (dtype, B, C, captured, kv)
    if key not in _RUNS:
        kw = {} if kv is None else dict(kv=kv, kv_chunk=True) if C else dict(kv=kv)
        _RUNS[key] = _chunk_run(_model(dtype), *_tokens(B), PRE, B, C, captured, **kw)
    return _RUNS[key]


def _restate(model, dec, tokens, pos, lo, hi):
    """fp32 restatement of the step that fed positions [lo, hi): O.transformer_layer's order, keys / values of every layer from the
    decoder's cache (slots [0, hi)), row j attending slots <= lo + j, the Sandwich-LN scale over the step's rows -> logits [B, hi - lo, V]"""
    B, C = tokens.shape[0], hi - lo
    p = {k: v.float().cpu() for k, v in model.module.state_dict().items()}
    caches = [c[:, :hi].cpu() for c in dec.kv8.dequantize()]
    assert all(bool(torch.isfinite(c).all()) for c in caches)
    x = torch.nn.functional.embedding(tokens[:, lo:hi].cpu(), p["word_embeddings.weight"]) \
        + torch.nn.functional.embedding(pos[:, lo:hi].cpu(), p["transformer.position_embeddings.weight"])
    split = lambda t, n: t.reshape(B, n, NH_, 64).permute(0, 2, 1, 3)
    mask = O.build_mask(C, hi)
    for l in range(L_):
        pre = f"transformer.layers.{l}."
        ln = lambda t, name: O.sandwich_layernorm(t, p[pre + name + ".weight"], p[pre + name + ".bias"])
        a = ln(x, "input_layernorm")
        q = O.linear(a, p[pre + "attention.query_key_value.weight"], p[pre + "attention.query_key_value.bias"])[..., :H_]
        k, v = caches[l][:, :, :H_], caches[l][:, :, H_:]
        ctx = O.standard_attention(split(q, C), split(k, hi), split(v, hi), mask)
        att = O.linear(ctx.permute(0, 2, 1, 3).reshape(B, C, H_), p[pre + "attention.dense.weight"], p[pre + "attention.dense.bias"])
        y = x + ln(att, "third_layernorm")
        c = ln(y, "post_attention_layernorm")
        m = O.linear(O.gelu(O.linear(c, p[pre + "mlp.dense_h_to_4h.weight"], p[pre + "mlp.dense_h_to_4h.bias"])),
                     p[pre + "mlp.dense_4h_to_h.weight"], p[pre + "mlp.dense_4h_to_h.bias"])
        x = y + ln(m, "fourth_layernorm")
    x = O.sandwich_layernorm(x, p["transformer.final_layernorm.weight"], p["transformer.final_layernorm.bias"])
    return O.linear(x, p["word_embeddings.weight"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", SHAPES)
def test_captured_chunk_step_equals_eager_and_matches_the_fp32_restatement_on_the_decoders_cache(dtype, B, C):
    from cogview_amd import functional as F_
    model = _model(dtype)
    tr = model.module.transformer
    assert F_.decode_chain_supported(tr, 4) and not F_.decode_chain_supported(tr, 8)
    dec_e, eager = _run(dtype, B, C, False)
    dec, graph = _run(dtype, B, C, True)
    assert dec.kv8 is not None and dec.caches is None and all(s.chunk for s in dec.slots)
    assert eager.shape == (B, CHUNKED + AFTER, V_) and eager.dtype == dtype and bool(torch.isfinite(eager.float()).all())
    assert torch.equal(graph, eager), "graph replay must reproduce the eager chunk step bit for bit"
    assert all(torch.equal(a, b) for a, b in zip(dec.kv8.tensors(), dec_e.kv8.tensors())), "and leave the same cache"
    tokens, pos = _tokens(B)
    lo = PRE + CHUNKED - C                                     # the last chunk step
    e_chunk = rel(graph[:, CHUNKED - C:CHUNKED], _restate(model, dec, tokens, pos, lo, lo + C))
    e_after = rel(graph[:, -1:], _restate(model, dec, tokens, pos, N - 1, N))
    print(f"[{dtype}] batch {B} chunk {C}: last chunk step vs fp32 restatement on the decoder's cache rel-L2 {e_chunk:.2e}, "
          f"last one-token step after the chunks {e_after:.2e}")
    assert e_chunk < TOL[dtype] and e_after < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", SHAPES)
def test_chunk_steps_move_the_logits_less_than_the_8bit_cache_itself(dtype, B, C):
    """A chunk step changes layer inputs in the last bits only (the Sandwich scale spans the chunk's rows), which can flip a few
    E4M3 roundings; that must be small next to quantizing every key and value: chunk-kv8 against one-token-kv8 does not exceed
    one-token-kv8 against one-token-16-bit, on the same tokens."""
    _, chunk8 = _run(dtype, B, C, False)
    _, one8 = _run(dtype, B, 0, False)
    _, one16 = _run(dtype, B, 0, False, kv=None)
    e_chunk, e_kv8 = rel(chunk8, one8), rel(one8, one16)
    print(f"[{dtype}] batch {B} chunk {C}: chunk steps on the 8-bit cache vs its one-token steps rel-L2 {e_chunk:.2e}; "
          f"one-token steps on the 8-bit cache vs on the 16-bit cache {e_kv8:.2e}")
    assert e_chunk <= e_kv8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weights", ["e4m3", "mxfp4"])
def test_chunk_steps_on_quantized_weights_match_the_one_token_decoder_of_the_same_form(dtype, weights):
    if weights == "mxfp4":
        from tests.test_w4_decode_gpu import _model as model_of
    else:
        from tests.test_w8_decode_gpu import _model as model_of
    model = model_of(dtype)                                    # 128 positions
    tokens, pos = _tokens(1, n=64)
    pre = 30
    _, ref = _chunk_run(model, tokens, pos, pre, 1, 0, False, capacity=128, weights=weights, kv="e4m3")
    res = {}
    for captured in (False, True):
        dec, res[captured] = _chunk_run(model, tokens, pos, pre, 1, 4, captured, capacity=128, weights=weights, kv="e4m3", kv_chunk=True)
        assert dec.wq is not None and dec.kv8 is not None
        e = rel(res[captured], ref)
        print(f"[{dtype}] weights={weights} chunk 4 captured={captured}: chunk steps on the 8-bit cache vs the one-token decoder rel-L2 {e:.2e}")
        assert bool(torch.isfinite(res[captured].float()).all()) and e < TOL[dtype]
    assert torch.equal(res[True], res[False])


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_steps_on_a_ragged_decoder_match_its_one_token_steps(dtype):
    """two prompts of 117 and 111 tokens right-aligned in one decoder (ragged=True): chunk steps of 4 per cache row against the
    one-token steps of the same decoder form"""
    model = _model(dtype)
    tokens, _ = _tokens(2)
    pads, P = [0, 6], PRE
    pos = torch.stack([torch.arange(N, device="cuda") - p for p in pads]).clamp(min=0)          # each prompt counts from its own start
    res = {}
    for C in (0, 4):
        dec = GraphDecoder(model, batch=2, capacity=CAP, ragged=True, chunk=C, kv="e4m3", **({"kv_chunk": True} if C else {}))
        with torch.no_grad():
            dec._prefill(tokens[:, :P].clone(), pos[:, :P].clone(), None, pads)
        assert dec.first.tolist() == pads
        step = C or 1
        outs = []
        for t in range(P, P + CHUNKED, step):
            outs.append((dec.step_chunk if C else dec.step)(tokens[:, t:t + step], pos[:, t:t + step]).clone())
        res[C] = torch.cat(outs, 1)
    e = rel(res[4], res[0])
    print(f"[{dtype}] ragged, chunk 4 on the 8-bit cache against its one-token steps: rel-L2 {e:.2e}")
    assert bool(torch.isfinite(res[4].float()).all()) and e < TOL[dtype]


# ----------------------------------------------------------------------------------------------------------------- the fillers
def _sequences(ids):
    """a run of 40 positions with 16 and 2 given ids inside it, and a shorter sequence with a shorter context"""
    ctx = _context(ids)
    g = torch.Generator().manual_seed(2)
    run = torch.full((40,), -1, dtype=torch.long)
    run[4:20] = torch.randint(0, N_IMG, (16,), generator=g)
    run[26:28] = torch.randint(0, N_IMG, (2,), generator=g)
    return torch.tensor(ctx + run.tolist(), device="cuda"), torch.tensor(ctx[2:] + run[:24].tolist(), device="cuda")


def _planned_calls(seq, ids, C):
    plan = plan_device_fill(seq.tolist(), ids, V_)
    widths = plan_chunk_steps(plan["given"], plan["context"], plan["replays"], C)
    return len(widths), sum(1 for w in widths if w > 1), plan["replays"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_filler_in_chunks_on_the_8bit_cache(dtype):
    """two calls per filler, the second on a SHORTER sequence (the slots the first call wrote past it are stale and must not
    matter): captured equals eager, given ids are kept, the model calls are the planned ones"""
    ids = ToyIds(N_IMG, N_TXT)
    seq, short = _sequences(ids)
    model, args = _model(dtype), _args()
    res = []
    for cap in (True, False):
        f = DeviceFiller(model, args, seed=77, capacity=128, capture=cap, chunk=8, kv="e4m3", kv_chunk=True)
        calls = []
        for s in (seq, short):
            out = f(model, s.clone(), args, tokenizer=ids)
            n_calls, n_chunks, replays = _planned_calls(s, ids, 8)
            assert f.model_calls == n_calls < replays and n_chunks > 0
            calls.append((out, f.scores))
        assert f.dec.kv8 is not None and f.dec.caches is None and f.dec.chunk == 8 and all(s_.chunk for s_ in f.dec.slots)
        assert f.dec.chunk_steps == sum(_planned_calls(s, ids, 8)[1] for s in (seq, short))
        assert (f.dec.graph_chunk is not None) == cap
        res.append(calls)
    for which, s in ((0, seq), (1, short)):
        (o_g, sc_g), (o_e, sc_e) = res[0][which], res[1][which]
        given = s >= 0
        assert torch.equal(o_g[0][given], s[given])
        assert int(o_g[0][~given].min()) >= 0 and int(o_g[0][~given].max()) < N_IMG
        assert sc_g.shape == (1,) and bool(torch.isfinite(sc_g).all()) and float(sc_g) < 0
        assert torch.equal(o_g, o_e) and torch.equal(sc_g, sc_e), which


def test_reused_chunk_filler_on_the_8bit_cache_equals_a_fresh_one():
    ids = ToyIds(N_IMG, N_TXT)
    seq, short = _sequences(ids)
    long_seq = torch.tensor(_context(ids) + [-1] * 44, device="cuda")
    model = _model(torch.float16)
    greedy = types.SimpleNamespace(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0)
    kw = dict(capacity=128, chunk=8, kv="e4m3", kv_chunk=True)
    reused = DeviceFiller(model, greedy, **kw)
    reused(model, long_seq.clone(), greedy, tokenizer=ids)
    assert reused.dec.chunk_steps == 0
    a = reused(model, short.clone(), greedy, tokenizer=ids)
    assert reused.dec.chunk_steps == _planned_calls(short, ids, 8)[1] > 0
    fresh = DeviceFiller(model, greedy, **kw)
    b = fresh(model, short.clone(), greedy, tokenizer=ids)
    assert torch.equal(a, b) and torch.equal(reused.scores, fresh.scores)


def test_batch_filler_in_chunks_on_the_8bit_cache():
    """DeviceBatchFiller(rows=2, chunk=4, kv="e4m3", kv_chunk=True): captured equals eager, given ids kept, the planned model calls"""
    from cogview_amd.generation import plan_device_batch_fill
    from tests.test_batch_fill_gpu import _captured_and_eager, _h1024, _sampled, _small_windows
    model, ids, n_img, n_txt = _h1024()
    seqs = _small_windows(ids, n_img, n_txt, (9, 4))
    plan = plan_device_batch_fill([s.tolist() for s in seqs], ids, V_)
    widths = plan_chunk_steps(plan["pattern"], plan["P"], plan["replays"], 4)
    outs, scores, f = _captured_and_eager(model, seqs, ids, _sampled(), 2, capacity=64, chunk=4, kv="e4m3", kv_chunk=True)
    assert f.model_calls == len(widths) < plan["replays"] and f.dec.chunk_steps == sum(1 for w in widths if w > 1) > 0
    assert f.dec.kv8 is not None and f.dec.graph is not None and f.dec.graph_chunk is not None and all(s.chunk for s in f.dec.slots)
    assert bool(torch.isfinite(scores).all()) and bool((scores < 0).all())
    for seq, out in zip(seqs, outs):
        assert int(out[0][seq < 0].min()) >= 0 and int(out[0][seq < 0].max()) < n_img
