"""GPU: the decode step of 9 .. 64 rows (functional.decode_layers(wide=True) behind GraphDecoder._step, ops.gemm_rows).
The decode attention and the sampler are untouched by it, but had no test above 8 rows: the attention at 17 and 64 rows against
the one-row call, on both cache formats, with and without `first`.  Then the 3-layer model of
test_fused_decode_chain_matches_layer_by_layer_and_full_sequence at 12 and 33 rows against the full-sequence forward, captured
against eager, wide against the step with the switch off, the same on the 8-bit cache at 12 rows, and device generation with
12 rows (one prompt x 12, three prompts x 4)."""
import types

import pytest
import torch

from cogview_amd import functional as F_
from cogview_amd.generation import add_interlacing_beam_marks, generate_batch_on_device, generate_on_device
from tests.generation_cases import ToyIds, build_model, load_golden
from tests.test_w8_decode_gpu import TOL, rel

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
HEADS, CAP, POS = 8, 256, 140                    # the attended slots end in the second key split of 128
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def _first(B, ragged):
    return ((torch.arange(B, dtype=torch.int32) * 37) % (POS - 3)).cuda() if ragged else None


def _attended(B, first):
    """[B, CAP] bool: slots [first[b], POS) -- slot POS itself is written by the call"""
    s = torch.arange(CAP, device="cuda").unsqueeze(0)
    lo = first.long().unsqueeze(1) if first is not None else torch.zeros((B, 1), dtype=torch.long, device="cuda")
    return (s >= lo) & (s < POS)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "first"])
@pytest.mark.parametrize("B", [17, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_attention_rows_equal_the_one_row_call(ops, dtype, B, ragged):
    hp = HEADS * 64
    g = torch.Generator().manual_seed(B)
    qkv = torch.randn((B, 1, 3 * hp), generator=g).to(dtype).cuda()
    cache = torch.randn((B, CAP, 2 * hp), generator=g).to(dtype).cuda()
    first = _first(B, ragged)
    cache[~_attended(B, first)] = NAN
    pos = torch.tensor([POS], dtype=torch.int64, device="cuda")
    kw = lambda sl: {} if first is None else {"first": first[sl]}
    wide_cache = cache.clone()
    wide = ops.attention_decode(qkv, wide_cache, pos, HEADS, **kw(slice(None))).clone()
    assert torch.isfinite(wide.float()).all()
    for b in range(B):
        one_cache = cache[b:b + 1].clone()
        one = ops.attention_decode(qkv[b:b + 1], one_cache, pos, HEADS, **kw(slice(b, b + 1)))
        assert torch.equal(one[0], wide[b]), b
        assert torch.equal(one_cache[0, POS], wide_cache[b, POS]), b


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "first"])
@pytest.mark.parametrize("B", [17, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_attention_kv8_rows_equal_the_one_row_call(ops, dtype, B, ragged):
    hp = HEADS * 64
    g = torch.Generator().manual_seed(B + 1)
    qkv = torch.randn((B, 1, 3 * hp), generator=g).to(dtype).cuda()
    kv = torch.randn((B, CAP, 2 * hp), generator=g).to(dtype).cuda()
    q = torch.empty((B, 2, HEADS, CAP, 64), dtype=torch.uint8, device="cuda")
    scale = torch.empty((B, 2, HEADS, CAP), dtype=torch.float32, device="cuda")
    ops.kv_quantize_e4m3(kv, q, scale)
    first = _first(B, ragged)
    dead = ~_attended(B, first)                                   # [B, CAP]
    q.masked_fill_(dead.view(B, 1, 1, CAP, 1), 0x7F)              # the E4M3 NaN byte
    scale.masked_fill_(dead.view(B, 1, 1, CAP), NAN)
    pos = torch.tensor([POS], dtype=torch.int64, device="cuda")
    kw = lambda sl: {} if first is None else {"first": first[sl]}
    wq, ws = q.clone(), scale.clone()
    wide = ops.attention_decode_kv8(qkv, (wq, ws), pos, HEADS, **kw(slice(None))).clone()
    assert torch.isfinite(wide.float()).all()
    for b in range(B):
        oq, os_ = q[b:b + 1].clone(), scale[b:b + 1].clone()
        one = ops.attention_decode_kv8(qkv[b:b + 1], (oq, os_), pos, HEADS, **kw(slice(b, b + 1)))
        assert torch.equal(one[0], wide[b]), b
        assert torch.equal(oq[0, :, :, POS], wq[b, :, :, POS]) and torch.equal(os_[0, :, :, POS], ws[b, :, :, POS]), b


# ------------------------------------------------------------------------------------------------ model level
L_, V_, H_, NH_, S_ = 3, 1024, 512, 8, 40
PRE = S_ - 8
_MODELS, _RUNS = {}, {}


def _model(dtype):
    """the model of test_fused_decode_chain_matches_layer_by_layer_and_full_sequence"""
    if dtype not in _MODELS:
        from cogview_amd.fp16 import FP16_Module
        from cogview_amd.model import GPT2Model
        torch.manual_seed(11)
        m = GPT2Model(L_, V_, H_, NH_, 0.0, 0.0, 0.0, S_ + 1, 64, False)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.data.add_(0.1 * torch.randn_like(p))
        _MODELS[dtype] = FP16_Module(m.cuda(), dtype=dtype, keep_half_outputs=True).eval()
    return _MODELS[dtype]


def _tokens(B):
    tokens = torch.randint(0, V_, (B, S_), generator=torch.Generator().manual_seed(3)).cuda()
    return tokens, torch.arange(S_, device="cuda").unsqueeze(0).expand(B, -1)


def _run(dtype, B, wide, captured, kv=None):
    """prefill, then 8 steps: logits [B, 8, V]; wide=False: the step with functional._DECODE_WIDE off"""
    key = (dtype, B, wide, captured, kv)
    if key not in _RUNS:
        from cogview_amd.generation import GraphDecoder
        model = _model(dtype)
        tokens, pos = _tokens(B)
        saved = F_._DECODE_WIDE, F_._DECODE_WIDE_MAX_ROWS
        F_._DECODE_WIDE, F_._DECODE_WIDE_MAX_ROWS = wide, 64          # every row count the kernel takes, not only the default's
        try:
            assert F_.decode_wide_supported(model.module.transformer, B) == wide
            dec = GraphDecoder(model, batch=B, capacity=128, kv=kv)
            dec.prefill(tokens[:, :PRE], pos[:, :PRE])
            if captured:
                dec.capture()
            _RUNS[key] = torch.cat([dec.step(tokens[:, t:t + 1], pos[:, t:t + 1]).clone() for t in range(PRE, S_)], 1)
        finally:
            F_._DECODE_WIDE, F_._DECODE_WIDE_MAX_ROWS = saved
    return _RUNS[key]


@pytest.mark.parametrize("B", [12, 33])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_step_against_the_full_sequence_forward(dtype, B):
    tokens, pos = _tokens(B)
    with torch.no_grad():
        full, *_ = _model(dtype)(tokens, pos, 0, None, None, 0)
    eager, graph, narrow = _run(dtype, B, True, False), _run(dtype, B, True, True), _run(dtype, B, False, False)
    assert eager.shape == (B, S_ - PRE, V_) and eager.dtype == dtype
    e, e0, d = rel(eager, full[:, PRE:]), rel(narrow, full[:, PRE:]), rel(eager, narrow)
    print(f"[{dtype}] {B} rows: wide step vs full sequence rel-L2 {e:.2e} (switch off: {e0:.2e}); wide vs switch off {d:.2e}")
    assert e < TOL[dtype] and e0 < TOL[dtype] and d < TOL[dtype]
    assert torch.equal(graph, eager), "graph replay must reproduce the eager wide step bit for bit"


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_step_on_the_8bit_cache(dtype):
    eager, graph, narrow = (_run(dtype, 12, w, c, kv="e4m3") for w, c in ((True, False), (True, True), (False, False)))
    assert torch.isfinite(eager.float()).all()
    d = rel(eager, narrow)
    print(f"[{dtype}] 12 rows on the 8-bit cache: wide vs switch off rel-L2 {d:.2e}")
    assert d < TOL[dtype]
    assert torch.equal(graph, eager), "graph replay must reproduce the eager wide step bit for bit"


# ------------------------------------------------------------------------------------------------ generation
def _sampled():
    return types.SimpleNamespace(temperature=1.02, top_k=200, top_p=0.9, is_sparse=0)


def _check_rows(out, seq, nb, n_img):
    n = int((seq >= 0).sum())
    assert out.shape == (nb, seq.numel()) and torch.equal(out[:, :n], seq[:n].expand(nb, n))          # returned unpadded
    assert int(out[:, n:].min()) >= 0 and int(out[:, n:].max()) < n_img                               # the drawable range
    assert len({tuple(r) for r in out[:, n:].tolist()}) > 1, "independent rows drew identical sequences"


def test_twelve_rows_of_the_toy_golden_model_keep_the_step_they_had(golden_dir):
    """h = 256 is outside the wide kernel's shapes: nothing new is refused, the step is what it was"""
    z, c = load_golden(golden_dir)
    ids, model = ToyIds(c["img_tokens"], c["txt_tokens"]), build_model(z, c, "cuda", True)
    assert not F_.decode_wide_supported(model.module.transformer, 12)
    seq = torch.from_numpy(z["t2i_seq"]).cuda()
    add_interlacing_beam_marks(seq, nb=12)
    res = [generate_on_device(model, seq.clone(), _sampled(), tokenizer=ids, seed=1234, capture=cap) for cap in (True, False)]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][1].shape == (12,) and torch.isfinite(res[0][1]).all()
    _check_rows(res[0][0], seq, 12, c["img_tokens"])


def _h1024():
    from tests.test_batch_generation_gpu import _h1024 as h
    return h()


def test_generate_on_device_with_twelve_rows():
    model, ids, ctxs, n_img = _h1024()
    assert F_.decode_wide_supported(model.module.transformer, 12)
    seq = torch.tensor(ctxs[2] + [-1] * 16, dtype=torch.long, device="cuda")
    add_interlacing_beam_marks(seq, nb=12)
    res = [generate_on_device(model, seq.clone(), _sampled(), tokenizer=ids, seed=1234, capture=cap) for cap in (True, False)]
    assert torch.equal(res[0][0], res[1][0]), (res[0][0].tolist(), res[1][0].tolist())
    assert torch.equal(res[0][1], res[1][1]) and res[0][1].shape == (12,) and torch.isfinite(res[0][1]).all()
    _check_rows(res[0][0], seq, 12, n_img)


def test_generate_batch_on_device_three_prompts_times_four():
    from tests.test_batch_generation_gpu import _captured_equals_eager, _h1024_seqs
    model, ids, ctxs, n_img = _h1024()
    assert F_.decode_wide_supported(model.module.transformer, 12)
    _captured_equals_eager(model, ids, _h1024_seqs(ctxs, (0, 1, 2), 4), n_img, 4)
