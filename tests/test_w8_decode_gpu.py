"""GPU: the decode step on 8-bit weights -- GraphDecoder(weights="e4m3") and the callers that hand the keyword on.
A 2-layer model, h = 1024, 16 heads, vocabulary 8192 + 512, fp16 and bf16.

The model's Linear weights and its word-embedding matrix are SNAPPED before use: every row lies on the E4M3 grid times a
power-of-two row scale and carries an element of magnitude 448 * scale, so the quantizer reproduces them exactly
(q.float() * scale == the stored 16-bit weight).  The prefill runs on the 16-bit weights by design; without the snap the
keys / values it leaves in the cache would differ from the 8-bit model's by the quantization of the weights (percent), and a
comparison against an oracle on q.float() * scale would measure that instead of the kernels."""
import types

import pytest
import torch

from oracle import cogview_oracle as O
from tests.generation_cases import ToyIds

pytestmark = pytest.mark.gpu

L_, H_, NH_, N_IMG, N_TXT, P_ = 2, 1024, 16, 8192, 504, 128
V_ = N_IMG + N_TXT + 8                                     # 8192 + 512
PRE, STEPS = 40, 6
TOL = {torch.float16: 3e-3, torch.bfloat16: 3e-2}          # tests/test_model_gpu.py: the decode tests' bars
E4M3 = torch.float8_e4m3fn


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _snap(w):
    """rows onto the E4M3 grid with a power-of-two scale, the row maximum at 448 * scale"""
    amax = w.abs().amax(dim=1, keepdim=True)
    s = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    out = (w / s).to(E4M3).float() * s
    idx = w.abs().argmax(dim=1, keepdim=True)
    out.scatter_(1, idx, torch.sign(w.gather(1, idx)) * 448.0 * s)
    return out


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
                    p.add_(0.1 * torch.randn_like(p))              # non-trivial LayerNorm affine / biases
                elif "position_embeddings" not in n:
                    p.copy_(_snap(p))
                    assert torch.equal(p.to(dtype).float(), p), n  # the snapped values are 16-bit values
        _MODELS[dtype] = FP16_Module(m.cuda(), dtype=dtype, keep_half_outputs=True).eval()
    return _MODELS[dtype]


def _tokens(B):
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, V_, (B, PRE + STEPS), generator=g).cuda()
    pos = torch.arange(PRE + STEPS, device="cuda").unsqueeze(0).expand(B, -1)
    return tokens, pos


def _decode(model, B, fused=True, captured=False, weights="e4m3"):
    from cogview_amd.generation import GraphDecoder
    tokens, pos = _tokens(B)
    dec = GraphDecoder(model, batch=B, capacity=128, weights=weights)
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
    assert dec.w8 is not None and eager.shape == (B, STEPS, V_) and eager.dtype == dtype
    assert torch.isfinite(eager.float()).all()
    assert torch.equal(graph, eager), "graph replay must reproduce the eager 8-bit step bit for bit"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 4])
def test_chain_matches_layer_by_layer(dtype, B):
    """the criterion of test_fused_decode_chain_matches_layer_by_layer_and_full_sequence for the 16-bit pair"""
    _, chain = _run(dtype, B, True, False)
    _, layers = _run(dtype, B, False, False)
    e = rel(chain, layers)
    print(f"[{dtype}] batch {B}: 8-bit chain vs 8-bit layer by layer rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 4])
def test_last_logits_against_the_fp32_oracle_on_the_quantized_weights(dtype, B):
    from cogview_amd import ops
    model = _model(dtype)
    dec, out = _run(dtype, B, True, True)
    p = {k: v.float().cpu() for k, v in model.module.state_dict().items()}
    q = dict(p)
    for k, v in model.module.state_dict().items():
        if v.dim() == 2 and "position_embeddings" not in k:
            qq, sc = ops.quantize_rows_e4m3(v)
            q[k] = qq.cpu().view(E4M3).float() * sc.cpu()[:, None]
            assert torch.equal(q[k], p[k]), f"{k}: the snapped weight must survive the quantizer exactly"
    tokens, pos = _tokens(B)
    ids, pid = tokens.cpu(), pos.cpu()
    S = ids.shape[1]
    x = torch.nn.functional.embedding(ids, p["word_embeddings.weight"]) \
        + torch.nn.functional.embedding(pid, p["transformer.position_embeddings.weight"])       # the lookup table as stored
    mask = O.build_mask(S, S)
    for l in range(L_):
        x = O.transformer_layer(x, mask, q, f"transformer.layers.{l}.", NH_)
    x = O.sandwich_layernorm(x, p["transformer.final_layernorm.weight"], p["transformer.final_layernorm.bias"])
    ref = O.linear(x[:, -1], q["word_embeddings.weight"])
    e = rel(out[:, -1], ref)
    print(f"[{dtype}] batch {B}: captured 8-bit decode, last logits vs fp32 oracle on q * scale: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


def test_decoder_without_the_keyword_holds_no_8bit_tensors():
    from cogview_amd.generation import GraphDecoder, SamplingDecoder
    for cls in (GraphDecoder, SamplingDecoder):
        dec = cls(_model(torch.float16), batch=1, capacity=128)
        assert dec.w8 is None
        assert not [k for k, v in vars(dec).items() if isinstance(v, torch.Tensor) and v.dtype == torch.uint8]
    dec = GraphDecoder(_model(torch.float16), batch=1, capacity=128, weights="e4m3")
    assert len(dec.w8.layers) == L_ and all(t.dtype in (torch.uint8, torch.float32) for t in dec.w8.tensors())
    assert dec.w8.emb[0].shape == (V_, H_)


def _args():
    return types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.9, is_sparse=0)


def _context(ids):
    g = torch.Generator().manual_seed(9)
    text = (N_IMG + torch.randint(0, N_TXT, (6,), generator=g)).tolist()
    return text + [ids["[BASE]"], ids["[BOI1]"]]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_generate_on_device_with_8bit_weights(dtype):
    from cogview_amd.generation import add_interlacing_beam_marks, generate_on_device
    ids = ToyIds(N_IMG, N_TXT)
    ctx = _context(ids)
    seq = torch.tensor(ctx + [-1] * 16, device="cuda")
    add_interlacing_beam_marks(seq, nb=4)
    res = [generate_on_device(_model(dtype), seq.clone(), _args(), tokenizer=ids, seed=1234, capture=cap, weights="e4m3")
           for cap in (True, False)]
    out, scores = res[0]
    assert out.shape == (4, len(ctx) + 16) and scores.shape == (4,)
    assert int(out[:, len(ctx):].min()) >= 0 and int(out[:, len(ctx):].max()) < N_IMG
    assert torch.isfinite(scores).all()
    assert torch.equal(res[0][0], res[1][0]), (res[0][0].tolist(), res[1][0].tolist())
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_device_filler_with_8bit_weights(dtype):
    from cogview_amd.generation import DeviceFiller
    ids = ToyIds(N_IMG, N_TXT)
    ctx = _context(ids)
    g = torch.Generator().manual_seed(2)
    run = torch.full((24,), -1, dtype=torch.long)
    run[4:8] = torch.randint(0, N_IMG, (4,), generator=g)          # given ids inside the run
    run[15:17] = torch.randint(0, N_IMG, (2,), generator=g)
    seq = torch.tensor(ctx + run.tolist(), device="cuda")
    model, args = _model(dtype), _args()
    res = []
    for cap in (True, False):
        f = DeviceFiller(model, args, seed=77, capacity=128, capture=cap, weights="e4m3")
        res.append((f(model, seq.clone(), args, tokenizer=ids), f.scores))
        assert f.dec.w8 is not None
    out, given = res[0][0][0], seq >= 0
    assert torch.equal(out[given], seq[given])
    assert int(out[~given].min()) >= 0 and int(out[~given].max()) < N_IMG
    assert res[0][1].shape == (1,) and torch.isfinite(res[0][1]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
