"""GPU: the decode step of 9 .. 64 rows on quantized weights (GraphDecoder(weights=f, wide=True): functional.decode_layers(w8=...,
wide=True) on ops.gemm_rows_w8 / ops.gemm_rows_w4).  The 3-layer h = 512 model of tests/test_wide_decode_gpu.py at 12 and 33 rows,
both formats, both dtypes: the captured step equals the eager one bit for bit, and the logits of 8 steps stay within the decode
tests' bar (rel-L2) of the SAME rows decoded by the quantized decoder as it was, in groups of at most 8 rows -- the same quantized
weights; only the order of the sums and the scope of the Sandwich-LN abs-max (all rows of a step) differ.  The same at 12 rows on
the 8-bit cache.  Then device generation with nb = 12 on the h = 1024 model, the nine windows' filler at 9 rows, and a decoder built
without the keyword, which holds and launches what it did."""
import pytest
import torch

from cogview_amd.generation import DeviceBatchFiller, GraphDecoder, add_interlacing_beam_marks, generate_on_device
from tests.test_w8_decode_gpu import TOL, rel
from tests.test_wide_decode_gpu import PRE, S_, V_, _check_rows, _h1024, _model, _sampled, _tokens

pytestmark = pytest.mark.gpu

FORMATS = ("e4m3", "mxfp4")
DTYPES = [torch.float16, torch.bfloat16]
_RUNS = {}


def _steps(dec, tokens, pos):
    return torch.cat([dec.step(tokens[:, t:t + 1], pos[:, t:t + 1]).clone() for t in range(PRE, S_)], 1)


def _run(fmt, dtype, B, captured, kv=None):
    """prefill, then 8 steps of the wide quantized decoder: logits [B, 8, V]"""
    key = (fmt, dtype, B, captured, kv)
    if key not in _RUNS:
        tokens, pos = _tokens(B)
        dec = GraphDecoder(_model(dtype), batch=B, capacity=128, weights=fmt, kv=kv, wide=True)
        assert dec.wide_q
        dec.prefill(tokens[:, :PRE], pos[:, :PRE])
        if captured:
            dec.capture()
        _RUNS[key] = _steps(dec, tokens, pos)
    return _RUNS[key]


def _in_groups(fmt, dtype, B, kv=None):
    """the same rows through the quantized decoder without the keyword, at most 8 rows at a time"""
    tokens, pos = _tokens(B)
    out = []
    for r0 in range(0, B, 8):
        n = min(8, B - r0)
        dec = GraphDecoder(_model(dtype), batch=n, capacity=128, weights=fmt, kv=kv)
        assert not dec.wide_q
        dec.prefill(tokens[r0:r0 + n, :PRE], pos[r0:r0 + n, :PRE])
        out.append(_steps(dec, tokens[r0:r0 + n], pos[r0:r0 + n]))
    return torch.cat(out, 0)


@pytest.mark.parametrize("B", [12, 33])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_wide_quantized_step_against_groups_of_eight(fmt, dtype, B):
    eager, graph = _run(fmt, dtype, B, False), _run(fmt, dtype, B, True)
    assert eager.shape == (B, S_ - PRE, V_) and eager.dtype == dtype and torch.isfinite(eager.float()).all()
    assert torch.equal(graph, eager), "graph replay must reproduce the eager step bit for bit"
    d = rel(eager, _in_groups(fmt, dtype, B))
    print(f"[{fmt} {dtype}] {B} rows: wide quantized step vs groups of at most 8 rows rel-L2 {d:.2e}")
    assert d < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_wide_quantized_step_on_the_8bit_cache(fmt, dtype):
    eager, graph = _run(fmt, dtype, 12, False, kv="e4m3"), _run(fmt, dtype, 12, True, kv="e4m3")
    assert torch.isfinite(eager.float()).all()
    assert torch.equal(graph, eager), "graph replay must reproduce the eager step bit for bit"
    d = rel(eager, _in_groups(fmt, dtype, 12, kv="e4m3"))
    print(f"[{fmt} {dtype}] 12 rows on the 8-bit cache: wide quantized step vs groups of at most 8 rows rel-L2 {d:.2e}")
    assert d < TOL[dtype]


@pytest.mark.parametrize("fmt", FORMATS)
def test_generate_on_device_with_twelve_rows(fmt):
    model, ids, ctxs, n_img = _h1024()
    seq = torch.tensor(ctxs[2] + [-1] * 16, dtype=torch.long, device="cuda")
    add_interlacing_beam_marks(seq, nb=12)
    with pytest.raises(NotImplementedError, match="> 8 rows"):
        generate_on_device(model, seq.clone(), _sampled(), tokenizer=ids, seed=1234, weights=fmt)
    res = [generate_on_device(model, seq.clone(), _sampled(), tokenizer=ids, seed=1234, capture=cap, weights=fmt, wide=True) for cap in (True, False)]
    assert torch.equal(res[0][0], res[1][0]), (res[0][0].tolist(), res[1][0].tolist())
    assert torch.equal(res[0][1], res[1][1]) and res[0][1].shape == (12,) and torch.isfinite(res[0][1]).all()
    _check_rows(res[0][0], seq, 12, n_img)


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_filler_with_nine_rows(fmt):
    """the windows of tests/test_batch_fill_gpu.py::test_nine_rows_on_the_wide_step, on the quantized weights"""
    from tests import test_batch_fill_gpu as BF
    model, ids, n_img, n_txt = BF._h1024()
    seqs = BF._small_windows(ids, n_img, n_txt, (9, 4, 7, 1, 3, 11, 2, 5, 8), seed=80)
    outs, scores, f = BF._captured_and_eager(model, seqs, ids, BF._sampled(), 9, capacity=64, weights=fmt, wide=True)
    assert f.dec.wide_q and f.dec.wq is not None
    assert scores.shape == (9,) and torch.isfinite(scores).all()
    for seq, out in zip(seqs, outs):
        assert int(out[0][seq < 0].min()) >= 0 and int(out[0][seq < 0].max()) < n_img
    assert len({tuple(out[0][seq < 0].tolist()) for seq, out in zip(seqs, outs)}) == 9
    with pytest.raises(NotImplementedError, match=f"weights='{fmt}'"):
        DeviceBatchFiller(model, BF._args(), rows=9, capacity=64, weights=fmt)


def _one_step(dec, B):
    tokens, pos = _tokens(B)
    dec.prefill(tokens[:, :PRE], pos[:, :PRE])
    return dec.step(tokens[:, PRE:PRE + 1], pos[:, PRE:PRE + 1]).clone()


def _held(dec):
    return sorted((k, tuple(v.shape), v.dtype) for k, v in vars(dec).items() if isinstance(v, torch.Tensor))


def test_a_decoder_without_the_keyword_holds_and_launches_what_it_did():
    model = _model(torch.float16)
    # 16-bit weights at 12 rows: the keyword has no effect
    plain, keyed = GraphDecoder(model, batch=12, capacity=128), GraphDecoder(model, batch=12, capacity=128, wide=True)
    assert not plain.wide_q and not keyed.wide_q and keyed.wq is None and _held(plain) == _held(keyed)
    assert not [k for k, v in vars(plain).items() if isinstance(v, torch.Tensor) and v.dtype == torch.uint8]
    assert torch.equal(_one_step(plain, 12), _one_step(keyed, 12))
    for fmt in FORMATS:
        # quantized weights up to 8 rows: the skinny step, with or without the keyword
        plain, keyed = (GraphDecoder(model, batch=8, capacity=128, weights=fmt, **kw) for kw in ({}, {"wide": True}))
        assert not plain.wide_q and not keyed.wide_q and _held(plain) == _held(keyed)
        assert torch.equal(_one_step(plain, 8), _one_step(keyed, 8))
        # above 8 rows without it: refused as ever, before anything is quantized
        with pytest.raises(NotImplementedError) as e:
            GraphDecoder(model, batch=12, capacity=128, weights=fmt)
        assert str(e.value) == f"weights={fmt!r}: batch 12 > 8 rows"
