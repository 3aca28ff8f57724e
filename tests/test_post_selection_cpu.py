"""Post-selection on the device, the parts that need no GPU: post_selection_rows' layout and refusals, the reference's chunking
rule, the refusals of inverse_prompt_score_on_device that come before the model is touched, the binding's descriptor, and the
host logic of the device score on the CPU-emulated ops (tests/cpu_ops.py, as tests/test_generation_cpu.py uses them) with a torch
stand-in for ops.score_targets -- held to the reference's own scores (tests/golden/generate_samples.npz)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cpu_ops
from tests.generation_cases import ToyIds, build_model
from tests.post_selection_cases import IMAGE_TOKENS, SCORE_ATOL, generated_rows, golden_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def score_targets_torch(logits, targets, allow=None, group=1, logp=None, scores=None):
    """ops.score_targets in torch: log_softmax over the allowed slice in fp32, gather, -inf for a target outside, group sums."""
    v = logits.shape[-1]
    lo, hi = (0, v) if allow is None else allow
    x = logits.reshape(-1, v).float()
    t = targets.reshape(-1)
    assert x.shape[0] == t.numel() and x.shape[0] % group == 0
    inside = (t >= lo) & (t < hi)
    lp = torch.log_softmax(x[:, lo:hi], dim=-1).gather(1, (t - lo).clamp(0, hi - lo - 1).unsqueeze(1)).squeeze(1)
    lp = torch.where(inside, lp, torch.full_like(lp, -float("inf")))
    sc = lp.view(-1, group).sum(dim=1)
    if logp is not None:
        logp.copy_(lp)
    if scores is not None:
        scores.copy_(sc)
    return (lp if logp is None else logp), (sc if scores is None else scores)


@pytest.fixture()
def cpu_kernels(monkeypatch):
    import torch.distributed as dist
    from cogview_amd import mpu, ops
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % (29900 + os.getpid() % 90), world_size=1, rank=0)
    if not mpu.model_parallel_is_initialized():
        mpu.initialize_model_parallel(1)
    cpu_ops.install(monkeypatch.setattr)
    monkeypatch.setattr(ops, "score_targets", score_targets_torch)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    yield


def _rows(ids, texts, codes):
    return torch.stack([torch.tensor([ids["[ROI1]"]] + t + [ids["[BASE]"], ids["[BOI1]"]] + c) for t, c in zip(texts, codes)])


def test_post_selection_rows_layout():
    from cogview_amd.generation import post_selection_rows
    ids = ToyIds(8192, 500)
    texts, codes = [[8200, 8201, 8202], [8300, 8301, 8302]], [[1, 2, 3, 4], [5, 6, 7, 8191]]
    out = post_selection_rows(_rows(ids, texts, codes), ids, image_tokens=4)
    assert out.dtype == torch.int64 and tuple(out.shape) == (2, 2 + 4 + 1 + 1 + 3)
    for r in range(2):
        assert out[r].tolist() == [ids["[BASE]"], ids["[BOI1]"]] + codes[r] + [ids["[EOI1]"], ids["[ROI1]"]] + texts[r]
    # no text at all is still a layout (the score refuses it, not the rebuilding)
    assert post_selection_rows(_rows(ids, [[]], [[1, 2, 3, 4]]), ids, image_tokens=4).tolist() == \
        [[ids["[BASE]"], ids["[BOI1]"], 1, 2, 3, 4, ids["[EOI1]"], ids["[ROI1]"]]]


def test_post_selection_rows_refuses_other_layouts():
    from cogview_amd.generation import post_selection_rows
    ids = ToyIds(8192, 500)
    good = _rows(ids, [[8200, 8201], [8300, 8301]], [[1, 2, 3, 4], [5, 6, 7, 8]])
    post_selection_rows(good, ids, image_tokens=4)
    for col, val in ((0, ids["[BASE]"]), (3, ids["[ROI1]"]), (4, 8200), (6, -1), (8, 8192)):
        bad = good.clone()
        bad[1, col] = val                                 # the SECOND row only: every row is checked
        with pytest.raises(ValueError):
            post_selection_rows(bad, ids, image_tokens=4)
    with pytest.raises(ValueError):
        post_selection_rows(good, ids, image_tokens=5)    # the markers sit one column off
    with pytest.raises(ValueError):
        post_selection_rows(good[:, :6], ids, image_tokens=4)      # shorter than [ROI1] [BASE] [BOI1] + codes
    with pytest.raises(ValueError):
        post_selection_rows(good[0], ids, image_tokens=4)


def test_chunking_follows_the_reference_rule():
    """generate_samples.py post_selection: `num < mbz or num % mbz == 0`, then max(num // mbz, 1) blocks of mbz rows."""
    from cogview_amd.generation.sampling import _score_chunks
    assert _score_chunks(8, None) == [(0, 8)]
    assert _score_chunks(8, 8) == [(0, 8)]
    assert _score_chunks(8, 4) == [(0, 4), (4, 8)]
    assert _score_chunks(3, 8) == [(0, 3)]
    assert _score_chunks(2, 1) == [(0, 1), (1, 2)]
    for num, mbz in ((6, 4), (9, 8), (8, 0), (8, -2)):
        with pytest.raises(ValueError):
            _score_chunks(num, mbz)


def test_refusals_come_before_the_model():
    from cogview_amd.generation import inverse_prompt_score_on_device
    ids = ToyIds(8192, 500)
    row = [ids["[BASE]"], ids["[BOI1]"], 1, 2, 3, 4, ids["[EOI1]"], ids["[ROI1]"], 8200, 8201]
    seq = torch.tensor([row, row])
    dense = types.SimpleNamespace(is_sparse=0)
    with pytest.raises(NotImplementedError, match="inverse_prompt_score"):
        inverse_prompt_score_on_device(None, seq, types.SimpleNamespace(is_sparse=2), tokenizer=ids, image_tokens=4)
    bad = seq.clone()
    bad[1, 7] = 8199                                       # [ROI1] missing in the second row only
    with pytest.raises(ValueError, match="ROI1"):
        inverse_prompt_score_on_device(None, bad, dense, tokenizer=ids, image_tokens=4)
    with pytest.raises(ValueError, match="no text"):
        inverse_prompt_score_on_device(None, seq[:, :8], dense, tokenizer=ids, image_tokens=4)


def test_score_desc_follows_the_header():
    from cogview_amd import _lib
    src = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    body = re.search(r"typedef struct cogv_score_desc \{(.*?)\} cogv_score_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", d)[-1] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.ScoreDesc._fields_]
    assert "cogv_score_targets" in _lib.SIGNATURES and hasattr(_lib.lib(), "cogv_score_targets")


def test_score_targets_has_no_cpu_fallback():
    from cogview_amd import _lib, ops
    with pytest.raises(_lib.CogviewHipError):
        ops.score_targets(torch.zeros(2, 16, dtype=torch.float16), torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize("kv_cache", [False, True])
def test_device_score_host_logic_reproduces_the_reference_scores(cpu_kernels, golden_dir, kv_cache):
    """[ROI1] check, embed + transformer, hidden states cut to the text positions before the tied projection, targets =
    the next tokens, image codes excluded, one group per row; unchunked and one row per forward."""
    from cogview_amd.generation import inverse_prompt_score_on_device, post_selection_rows, rerank_generated
    z, c, ids, args = golden_case(golden_dir)
    model = build_model(z, c, "cpu", kv_cache)
    sel = torch.from_numpy(z["sel_seq"])
    for max_rows in (None, 1):
        scores = inverse_prompt_score_on_device(model, sel, args, tokenizer=ids, max_rows=max_rows)
        assert scores.dtype == torch.float32 and tuple(scores.shape) == (2,)
        print("max_rows", max_rows, "scores", scores.tolist(), "golden", z["sel_scores"].tolist())
        assert np.allclose(scores.numpy(), z["sel_scores"], rtol=0, atol=SCORE_ATOL), (scores.tolist(), z["sel_scores"].tolist())
    args.max_inference_batch_size = 1                      # the default of max_rows
    assert torch.equal(inverse_prompt_score_on_device(model, sel, args, tokenizer=ids), scores)
    del args.max_inference_batch_size
    rows = generated_rows(z, ids, "cpu")
    assert torch.equal(post_selection_rows(rows, ids, IMAGE_TOKENS), sel)
    best, sc, order = rerank_generated(model, rows, args, tokenizer=ids)
    assert order.tolist() == [1, 0] and torch.equal(best, rows[[1, 0]])
    assert np.allclose(sc.numpy(), z["sel_scores"][[1, 0]], rtol=0, atol=SCORE_ATOL)
    best, sc, order = rerank_generated(model, rows, args, tokenizer=ids, keep=1)
    assert order.tolist() == [1] and torch.equal(best, rows[1:2]) and tuple(sc.shape) == (1,)
