"""GPU: the decode step on 4-bit weights -- GraphDecoder(weights="mxfp4") and the callers that hand the keyword on, on the small
models and with the bars of tests/test_w8_decode_gpu.py (2 layers, h = 1024, 16 heads, vocabulary 8192 + 512, fp16 and bf16).

As there, the model's Linear weights and its word-embedding matrix are SNAPPED before use, here onto the MXFP4 grid: every block of
32 lies on E2M1 codes times a power-of-two scale and carries an element of magnitude 4 * scale, so the quantizer reproduces the
weights exactly.  The prefill runs on the 16-bit weights by design; without the snap the keys / values it leaves in the cache
would differ from the 4-bit model's by the quantization of the weights, and the comparison against an oracle on the dequantized
weights would measure that instead of the kernels."""
import types

import pytest
import torch

from oracle import cogview_oracle as O
from tests import w4_cases as W4
from tests.generation_cases import ToyIds
from tests.test_w8_decode_gpu import L_, H_, NH_, N_IMG, N_TXT, P_, V_, PRE, STEPS, TOL, rel, _tokens, _args, _context

pytestmark = pytest.mark.gpu


def _snap(w):
    """blocks of 32 onto the MXFP4 grid: quantize, dequantize, and put 4 * 2^e with the sign of the block's largest element in its
    place, so that the quantizer finds the same scale again"""
    q, s = W4.quantize(w)
    out = W4.dequantize(q, s).float()
    N, K = w.shape
    blocks = w.view(N, K // 32, 32)
    idx = blocks.abs().argmax(dim=-1, keepdim=True)
    top = torch.sign(blocks.gather(-1, idx)) * 4.0 * torch.exp2(s.float() - 127).unsqueeze(-1)
    return out.view(N, K // 32, 32).scatter(-1, idx, top).view(N, K)


_MODELS = {}


def _model(dtype):
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
                    assert torch.equal(W4.dequantize(*W4.quantize(p)).float(), p), n
        _MODELS[dtype] = FP16_Module(m.cuda(), dtype=dtype, keep_half_outputs=True).eval()
    return _MODELS[dtype]


def _decode(model, B, fused=True, captured=False, **kw):
    from cogview_amd.generation import GraphDecoder
    tokens, pos = _tokens(B)
    dec = GraphDecoder(model, batch=B, capacity=128, weights="mxfp4", **kw)
    dec.fused = fused
    dec.prefill(tokens[:, :PRE], pos[:, :PRE])
    if captured:
        dec.capture()
    outs = [dec.step(tokens[:, t:t + 1], pos[:, t:t + 1]).clone() for t in range(PRE, PRE + STEPS)]
    return dec, torch.cat(outs, 1)


_RUNS = {}


def _run(dtype, B, fused, captured):
    key = (dtype, B, fused, captured)
    if key not in _RUNS:
        _RUNS[key] = _decode(_model(dtype), B, fused, captured)
    return _RUNS[key]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 4])
def test_captured_step_equals_the_eager_step(dtype, B):
    dec, eager = _run(dtype, B, True, False)
    _, graph = _run(dtype, B, True, True)
    assert dec.w4 is not None and dec.w8 is None and eager.shape == (B, STEPS, V_) and eager.dtype == dtype
    assert torch.isfinite(eager.float()).all()
    assert torch.equal(graph, eager), "graph replay must reproduce the eager 4-bit step bit for bit"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 4])
def test_chain_matches_layer_by_layer(dtype, B):
    _, chain = _run(dtype, B, True, False)
    _, layers = _run(dtype, B, False, False)
    e = rel(chain, layers)
    print(f"[{dtype}] batch {B}: 4-bit chain vs 4-bit layer by layer rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 4])
def test_last_logits_against_the_fp32_oracle_on_the_dequantized_weights(dtype, B):
    from cogview_amd import ops
    model = _model(dtype)
    dec, out = _run(dtype, B, True, True)
    p = {k: v.float().cpu() for k, v in model.module.state_dict().items()}
    q = dict(p)
    for k, v in model.module.state_dict().items():
        if v.dim() == 2 and "position_embeddings" not in k:
            q[k] = ops.dequantize_rows_mxfp4(*ops.quantize_rows_mxfp4(v)).cpu()
            assert torch.equal(q[k], p[k]), f"{k}: the snapped weight must survive the quantizer exactly"
    tokens, pos = _tokens(B)
    ids, pid = tokens.cpu(), pos.cpu()
    S = ids.shape[1]
    x = torch.nn.functional.embedding(ids, p["word_embeddings.weight"]) \
        + torch.nn.functional.embedding(pid, p["transformer.position_embeddings.weight"])
    mask = O.build_mask(S, S)
    for l in range(L_):
        x = O.transformer_layer(x, mask, q, f"transformer.layers.{l}.", NH_)
    x = O.sandwich_layernorm(x, p["transformer.final_layernorm.weight"], p["transformer.final_layernorm.bias"])
    ref = O.linear(x[:, -1], q["word_embeddings.weight"])
    e = rel(out[:, -1], ref)
    print(f"[{dtype}] batch {B}: captured 4-bit decode, last logits vs fp32 oracle on the dequantized weights: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


def test_decoder_without_the_keyword_holds_no_4bit_tensors():
    from cogview_amd.generation import GraphDecoder, SamplingDecoder
    for cls in (GraphDecoder, SamplingDecoder):
        dec = cls(_model(torch.float16), batch=1, capacity=128)
        assert dec.w4 is None and dec.w8 is None and dec.wq is None
        assert not [k for k, v in vars(dec).items() if isinstance(v, torch.Tensor) and v.dtype == torch.uint8]
    dec = GraphDecoder(_model(torch.float16), batch=1, capacity=128, weights="mxfp4")
    assert dec.w8 is None and len(dec.w4.layers) == L_ and all(t.dtype == torch.uint8 for t in dec.w4.tensors())
    assert dec.w4.emb[0].shape == (V_, H_ // 2) and dec.w4.emb[1].shape == (V_, H_ // 32)
    # 0.53 / 2 of the 16-bit bytes of the same matrices
    bytes4 = sum(t.numel() for t in dec.w4.tensors())
    bytes16 = 2 * sum(2 * q.numel() for lw in dec.w4.layers for q, _ in lw) + 2 * 2 * dec.w4.emb[0].numel()
    assert abs(bytes4 / bytes16 - 0.53125 / 2) < 1e-9


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_generate_on_device_with_4bit_weights(dtype):
    from cogview_amd.generation import add_interlacing_beam_marks, generate_on_device
    ids = ToyIds(N_IMG, N_TXT)
    ctx = _context(ids)
    seq = torch.tensor(ctx + [-1] * 16, device="cuda")
    add_interlacing_beam_marks(seq, nb=4)
    res = [generate_on_device(_model(dtype), seq.clone(), _args(), tokenizer=ids, seed=1234, capture=cap, weights="mxfp4")
           for cap in (True, False)]
    out, scores = res[0]
    assert out.shape == (4, len(ctx) + 16) and scores.shape == (4,)
    assert int(out[:, len(ctx):].min()) >= 0 and int(out[:, len(ctx):].max()) < N_IMG
    assert torch.isfinite(scores).all()
    assert torch.equal(res[0][0], res[1][0]), (res[0][0].tolist(), res[1][0].tolist())
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_device_filler_with_4bit_weights(dtype):
    from cogview_amd.generation import DeviceFiller
    ids = ToyIds(N_IMG, N_TXT)
    ctx = _context(ids)
    g = torch.Generator().manual_seed(2)
    run = torch.full((24,), -1, dtype=torch.long)
    run[4:8] = torch.randint(0, N_IMG, (4,), generator=g)
    run[15:17] = torch.randint(0, N_IMG, (2,), generator=g)
    seq = torch.tensor(ctx + run.tolist(), device="cuda")
    model, args = _model(dtype), _args()
    res = []
    for cap in (True, False):
        f = DeviceFiller(model, args, seed=77, capacity=128, capture=cap, weights="mxfp4")
        res.append((f(model, seq.clone(), args, tokenizer=ids), f.scores))
        assert f.dec.w4 is not None and f.dec.w8 is None
    out, given = res[0][0][0], seq >= 0
    assert torch.equal(out[given], seq[given])
    assert int(out[~given].min()) >= 0 and int(out[~given].max()) < N_IMG
    assert res[0][1].shape == (1,) and torch.isfinite(res[0][1]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------ with the other options
def _reference_step(dtype, B):
    """the plain 4-bit decoder's logits (eager chain), what the composed options are held against"""
    return _run(dtype, B, True, False)[1]


def test_composes_with_the_8bit_cache():
    """kv="e4m3" under weights="mxfp4": captured == eager to the bit, and the chain against layer by layer at the bar
    tests/test_kv8_decode_gpu.py holds that pair to."""
    dtype, B = torch.float16, 2
    _, eager = _decode(_model(dtype), B, True, False, kv="e4m3")
    dec, graph = _decode(_model(dtype), B, True, True, kv="e4m3")
    assert dec.w4 is not None and dec.kv8 is not None and dec.caches is None and torch.equal(graph, eager)
    assert torch.isfinite(eager.float()).all()
    e = rel(eager, _decode(_model(dtype), B, False, False, kv="e4m3")[1])
    print(f"4-bit weights on the e4m3 cache: chain vs layer by layer rel-L2 {e:.2e}")
    assert e < TOL[dtype]


def test_composes_with_ragged_rows():
    """ragged=True with first = 0 everywhere is the plain step: the same bits.  With a row's first slot moved that row's logits
    move, the other row's stay within the decode bar (the Sandwich scale of a step spans its rows, so they are not bit-equal), and
    the step agrees with the 16-bit ragged decoder on the same snapped weights at that bar."""
    dtype, B = torch.float16, 2
    from cogview_amd.generation import GraphDecoder
    tokens, pos = _tokens(B)
    plain = _run(dtype, B, True, True)[1]
    dec, ragged = _decode(_model(dtype), B, True, True, ragged=True)
    assert dec.first is not None and torch.equal(ragged, plain)
    outs = []
    for weights in ("mxfp4", None):
        dec2 = GraphDecoder(_model(dtype), batch=B, capacity=128, weights=weights, ragged=True)
        dec2.prefill(tokens[:, :PRE], pos[:, :PRE])
        dec2.first[1] = 7
        dec2.capture()
        outs.append(dec2.step(tokens[:, PRE:PRE + 1], pos[:, PRE:PRE + 1]).clone())
    out = outs[0]
    e0, e1, e16 = rel(out[0], plain[0, :1]), rel(out[1], plain[1, :1]), rel(out, outs[1])
    print(f"ragged 4-bit step, first = (0, 7): row 0 moved {e0:.2e}, row 1 moved {e1:.2e}; against the 16-bit ragged decoder {e16:.2e}")
    assert e0 < TOL[dtype] and not torch.equal(out[1], plain[1, :1]) and e1 > e0 and e16 < TOL[dtype]


def test_composes_with_chunk_steps():
    """chunk=4 under weights="mxfp4": the chunk step runs the 4-bit products on batch * 4 rows; captured == eager to the bit, and
    its logits agree with four one-token steps within the decode bar (the Sandwich scale of a chunk is taken over all its rows)."""
    dtype, B, Cn = torch.float16, 1, 4
    from cogview_amd.generation import GraphDecoder
    tokens, pos = _tokens(B)
    outs = []
    for captured in (False, True):
        dec = GraphDecoder(_model(dtype), batch=B, capacity=128, weights="mxfp4", chunk=Cn)
        dec.prefill(tokens[:, :PRE], pos[:, :PRE])
        if captured:
            dec.capture()
        outs.append(dec.step_chunk(tokens[:, PRE:PRE + Cn], pos[:, PRE:PRE + Cn]).clone())
    assert outs[0].shape == (B, Cn, V_) and torch.equal(outs[0], outs[1])
    e = rel(outs[0], _reference_step(dtype, B)[:, :Cn])
    print(f"4-bit chunk step vs four one-token steps: rel-L2 {e:.2e}")
    assert e < TOL[dtype]
