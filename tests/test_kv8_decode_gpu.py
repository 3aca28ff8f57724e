"""GPU: the decode step on the 8-bit key/value cache -- GraphDecoder(kv="e4m3"), alone and with weights="e4m3", and the callers
that hand the keyword on.  The model of tests/test_w8_decode_gpu.py (2 layers, h = 1024, 16 heads, weights snapped onto the E4M3
grid so that weights="e4m3" is exact), capacity 192: a prefill of 125 tokens and 6 teacher-forced steps, so the run crosses the
boundary between the first and the second 128-key split (slots 127 / 128).

The oracle comparison takes every layer's keys and values from the decoder's OWN cache (dequantize(), slots [0, pos]): two 16-bit
computations of the same key differ in the last bit now and then, which flips quantization bins and says nothing about the
kernels; with the keys and values shared, what remains between the decoder and the fp32 restatement is 16-bit arithmetic."""
import types

import pytest
import torch

from oracle import cogview_oracle as O
from tests.generation_cases import ToyIds
from tests.test_w8_decode_gpu import L_, H_, NH_, N_IMG, N_TXT, V_, TOL, _snap, rel

pytestmark = pytest.mark.gpu

CAP, PRE, STEPS = 192, 125, 6
DTYPES = [torch.float16, torch.bfloat16]


P_ = 192                                                   # positions: the run reaches 131
_MODELS = {}


def _model(dtype):
    """the model of tests/test_w8_decode_gpu.py with 192 positions"""
    if dtype not in _MODELS:
        from cogview_amd.fp16 import FP16_Module
        from cogview_amd.model import GPT2Model
        torch.manual_seed(5)
        m = GPT2Model(L_, V_, H_, NH_, 0.0, 0.0, 0.0, P_, P_, False)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
                elif "position_embeddings" not in n:
                    p.copy_(_snap(p))
                    assert torch.equal(p.to(dtype).float(), p), n
        _MODELS[dtype] = FP16_Module(m.cuda(), dtype=dtype, keep_half_outputs=True).eval()
    return _MODELS[dtype]


def _tokens(B):
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, V_, (1, PRE + STEPS), generator=g).expand(B, -1).contiguous().cuda()
    pos = torch.arange(PRE + STEPS, device="cuda").unsqueeze(0).expand(B, -1)
    return tokens, pos


_RUNS = {}


def _run(dtype, B, fused, captured, weights=None):
    key = (dtype, B, fused, captured, weights)
    if key not in _RUNS:
        from cogview_amd.generation import GraphDecoder
        tokens, pos = _tokens(B)
        dec = GraphDecoder(_model(dtype), batch=B, capacity=CAP, weights=weights, kv="e4m3")
        dec.fused = fused
        dec.prefill(tokens[:, :PRE], pos[:, :PRE])
        if captured:
            dec.capture()
        outs = [dec.step(tokens[:, t:t + 1], pos[:, t:t + 1]).clone() for t in range(PRE, PRE + STEPS)]
        _RUNS[key] = (dec, torch.cat(outs, 1))
    return _RUNS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 4, 8])
def test_captured_step_equals_the_eager_step(dtype, B):
    """B = 8 runs layer by layer (above COGV_DECODE_CHAIN_MAX_ROWS)"""
    dec, eager = _run(dtype, B, True, False)
    _, graph = _run(dtype, B, True, True)
    assert dec.kv8 is not None and dec.caches is None and eager.shape == (B, STEPS, V_) and eager.dtype == dtype
    assert torch.isfinite(eager.float()).all()
    assert torch.equal(graph, eager), "graph replay must reproduce the eager step bit for bit"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 4])
def test_chain_matches_layer_by_layer(dtype, B):
    _, chain = _run(dtype, B, True, False)
    _, layers = _run(dtype, B, False, False)
    e = rel(chain, layers)
    print(f"[{dtype}] batch {B}: chain vs layer by layer on the 8-bit cache rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weights", [None, "e4m3"])
def test_last_logits_against_the_fp32_restatement_on_the_decoders_cache(dtype, weights):
    B = 4
    model = _model(dtype)
    dec, out = _run(dtype, B, True, True, weights)
    p = {k: v.float().cpu() for k, v in model.module.state_dict().items()}
    tokens, pos = _tokens(B)
    last = PRE + STEPS - 1                                   # the slot of the last token
    assert dec.length == last + 1
    caches = [c[:, :last + 1].cpu() for c in dec.kv8.dequantize()]
    assert all(bool(torch.isfinite(c).all()) for c in caches)
    x = torch.nn.functional.embedding(tokens[:, last:].cpu(), p["word_embeddings.weight"]) \
        + torch.nn.functional.embedding(pos[:, last:].cpu(), p["transformer.position_embeddings.weight"])
    split = lambda t, n: t.reshape(B, n, NH_, 64).permute(0, 2, 1, 3)
    for l in range(L_):                                      # O.transformer_layer's order, keys / values from the decoder's cache
        pre = f"transformer.layers.{l}."
        ln = lambda t, name: O.sandwich_layernorm(t, p[pre + name + ".weight"], p[pre + name + ".bias"])
        a = ln(x, "input_layernorm")
        q = O.linear(a, p[pre + "attention.query_key_value.weight"], p[pre + "attention.query_key_value.bias"])[..., :H_]
        k, v = caches[l][:, :, :H_], caches[l][:, :, H_:]
        ctx = O.standard_attention(split(q, 1), split(k, last + 1), split(v, last + 1), torch.ones(1, 1, 1, last + 1))
        att = O.linear(ctx.permute(0, 2, 1, 3).reshape(B, 1, H_), p[pre + "attention.dense.weight"], p[pre + "attention.dense.bias"])
        y = x + ln(att, "third_layernorm")
        c = ln(y, "post_attention_layernorm")
        m = O.linear(O.gelu(O.linear(c, p[pre + "mlp.dense_h_to_4h.weight"], p[pre + "mlp.dense_h_to_4h.bias"])),
                     p[pre + "mlp.dense_4h_to_h.weight"], p[pre + "mlp.dense_4h_to_h.bias"])
        x = y + ln(m, "fourth_layernorm")
    x = O.sandwich_layernorm(x, p["transformer.final_layernorm.weight"], p["transformer.final_layernorm.bias"])
    ref = O.linear(x[:, -1], p["word_embeddings.weight"])
    e = rel(out[:, -1], ref)
    print(f"[{dtype}] weights={weights}: captured decode on the 8-bit cache, last logits vs fp32 restatement: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


def test_what_the_decoders_hold():
    from cogview_amd.generation import GraphDecoder, SamplingDecoder
    m = _model(torch.float16)

    def tensors(dec):
        out = [v for v in vars(dec).values() if isinstance(v, torch.Tensor)]
        out += [t for v in vars(dec).values() if isinstance(v, (list, tuple)) for t in v if isinstance(t, torch.Tensor)]
        if dec.kv8 is not None:
            out += dec.kv8.tensors() + [t for s in dec.slots for t in (s.q, s.scale)]
        return out

    for cls in (GraphDecoder, SamplingDecoder):
        dec = cls(m, batch=2, capacity=CAP)
        assert dec.kv8 is None and not [t for t in tensors(dec) if t.dtype == torch.uint8]
        dec = cls(m, batch=2, capacity=CAP, kv="e4m3")
        assert dec.caches is None and [t for t in tensors(dec) if t.dtype == torch.uint8]
        assert not [t for t in tensors(dec) if t.dtype in (torch.float16, torch.bfloat16) and tuple(t.shape[-3:]) == (2, CAP, 2 * H_)]
        assert not any(hasattr(s, "cache") for s in dec.slots)


def _args():
    return types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.9, is_sparse=0)


def _context(ids):
    g = torch.Generator().manual_seed(9)
    text = (N_IMG + torch.randint(0, N_TXT, (6,), generator=g)).tolist()
    return text + [ids["[BASE]"], ids["[BOI1]"]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weights", [None, "e4m3"])
def test_generate_on_device_with_the_8bit_cache(dtype, weights):
    from cogview_amd.generation import add_interlacing_beam_marks, generate_on_device
    ids = ToyIds(N_IMG, N_TXT)
    ctx = _context(ids)
    seq = torch.tensor(ctx + [-1] * 16, device="cuda")
    add_interlacing_beam_marks(seq, nb=4)
    res = [generate_on_device(_model(dtype), seq.clone(), _args(), tokenizer=ids, seed=1234, capture=cap, weights=weights, kv="e4m3")
           for cap in (True, False)]
    out, scores = res[0]
    assert out.shape == (4, len(ctx) + 16) and scores.shape == (4,)
    assert int(out[:, len(ctx):].min()) >= 0 and int(out[:, len(ctx):].max()) < N_IMG
    assert torch.isfinite(scores).all()
    assert torch.equal(res[0][0], res[1][0]), (res[0][0].tolist(), res[1][0].tolist())
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_filler_with_the_8bit_cache(dtype):
    """two calls per filler, the second on a SHORTER sequence: the slots the first call wrote past it are stale and must not matter"""
    from cogview_amd.generation import DeviceFiller
    ids = ToyIds(N_IMG, N_TXT)
    ctx = _context(ids)
    g = torch.Generator().manual_seed(2)
    run = torch.full((24,), -1, dtype=torch.long)
    run[4:8] = torch.randint(0, N_IMG, (4,), generator=g)          # given ids inside the run
    run[15:17] = torch.randint(0, N_IMG, (2,), generator=g)
    seq = torch.tensor(ctx + run.tolist(), device="cuda")
    short = torch.tensor(ctx[2:] + run[:12].tolist(), device="cuda")
    model, args = _model(dtype), _args()
    res = []
    for cap in (True, False):
        f = DeviceFiller(model, args, seed=77, capacity=128, capture=cap, kv="e4m3")
        first = (f(model, seq.clone(), args, tokenizer=ids), f.scores)
        second = (f(model, short.clone(), args, tokenizer=ids), f.scores)
        res.append((first, second))
        assert f.dec.kv8 is not None
    for which, s in ((0, seq), (1, short)):
        (o_g, sc_g), (o_e, sc_e) = res[0][which], res[1][which]
        given = s >= 0
        assert torch.equal(o_g[0][given], s[given])
        assert int(o_g[0][~given].min()) >= 0 and int(o_g[0][~given].max()) < N_IMG
        assert sc_g.shape == (1,) and torch.isfinite(sc_g).all()
        assert torch.equal(o_g, o_e) and torch.equal(sc_g, sc_e), which
